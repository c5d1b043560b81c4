"""Searchlight decoding: where in the brain is the task information?

At every centre a cross-validated classifier -- Gaussian naive Bayes, shrinkage LDA with ``classifier='lda'`` or a linear SVM
with ``classifier='svc'`` -- is fed only the centre's neighbourhood, and the centre gets the classifier's accuracy.
``searchlight`` does it on the device for any list of neighbourhoods -- ``graph.hop_balls`` of the brain graph for the classical
searchlight map, one row per parcel for ROI decoding, one row of all vertices for the whole-brain baseline a GCN accuracy is
reported against.  ``searchlight_events`` cuts the trial-mean patterns out of staged runs with ``match_events`` first.
``searchlight_host`` restates it in float64 NumPy, centre by centre.

The fit of naive Bayes is per-vertex moments and its decision a sum over the neighbourhood, so one fit per training set serves
every centre (chebgcn_searchlight_spread / _fit), and the work is the S x classes x sum |neighbourhood| likelihood terms of
chebgcn_searchlight_score.  All of it float64 in the centred form ``(x - mu)^2 / (2 sigma^2)``: see include/chebgcn.h.

Naive Bayes throws away that neighbouring vertices share noise; signal that lives in a difference of correlated vertices is
invisible to it.  ``classifier='lda'`` keeps it: every (training set, centre) pair gets its own pooled within-class covariance
of the ball, shrunk towards a multiple of the identity (a fixed ``shrinkage`` or Ledoit-Wolf's), its Cholesky factor and its
discriminants -- one workgroup per pair, everything on chip (chebgcn_searchlight_lda), for balls of up to ``LDA_PMAX``
vertices.  The model is stated once, in ``searchlight``'s docstring and in include/chebgcn.h.

Between the two sits a hole: ``'lda'`` refuses rows above ``LDA_PMAX`` vertices, and naive Bayes cannot use the covariance.
``classifier='svc'`` closes it: a one-vs-rest linear SVM per (training set, centre), solved in the dual by coordinate descent on
the n x n Gram matrix of the training samples (chebgcn_searchlight_svm, one workgroup per pair, everything on chip).  Its state
depends on the number of training samples (at most ``SVC_NMAX``) and not on the length of the row, so parcels of hundreds of
vertices and the whole-brain row are served.  Convergence is reported (``return_solver=True``: a ``SolverInfo``), never hidden.

Where the searchlight says WHERE the conditions can be told apart, ``crossnobis`` says HOW a region tells them apart: the
representational dissimilarity matrix of every ball -- the cross-validated Mahalanobis distance of every pair of classes per
(group, centre), whitened by the ball's shrunk noise covariance (chebgcn_searchlight_rdm, one workgroup per pair; the quantity
is stated once, in ``crossnobis``'s docstring and in include/chebgcn.h).  ``compare_rdms`` turns the RDMs into maps of agreement
with model RDMs for ``map_test``; ``crossnobis_events`` cuts the patterns from staged runs; ``crossnobis_host`` restates it
with SciPy.

Out of scope: SVM training sets above ``SVC_NMAX`` samples (a Gram matrix in HBM), non-linear kernels, one-vs-one or
Crammer-Singer multi-class, an unregularised bias, class weights, per-class covariances (QDA), balls above ``LDA_PMAX`` vertices
with ``'lda'`` or ``crossnobis``, returning the discriminant or primal weights, label-permutation nulls per subject (group
inference goes through ``map_test``), smoothing per ball (see ``searchlight``), temporal features beyond the trial mean,
any cleaning of the series, rank-based RDM comparisons (Spearman), noise ceilings and unbalanced designs in ``crossnobis``.

The host-only parts need NumPy and SciPy only.
"""
import collections
import types

import numpy as np
import scipy.sparse as sp

from . import runs as _runs
from .runs import host_array, is_tensor

CMAX, NMAX, GMAX = 32, 65535, 1 << 20           # chebgcn_searchlight_query(3), (5), (7)
SCORES_MAX_BYTES = 1 << 31                      # scores=True is refused beyond 2 GiB of float64 [S, classes, U]
FOLD_MAX = 16                                   # block_dura at most in searchlight_events (the indexed gather's fold)
LDA_PMAX = 128                                  # chebgcn_searchlight_lda_query(1): the longest row classifier='lda' serves
SHRINK_MIN = 1e-6                               # CHEBGCN_LDA_SHRINK_MIN: the floor of the shrinkage, given or estimated

SearchlightResult = collections.namedtuple('SearchlightResult', 'correct support recall accuracy groups classes scores predictions')
SearchlightResult.__doc__ = """What ``searchlight`` returns.  ``correct`` int32 [G, classes, U]: the test samples of group g and
class c that centre u classified correctly; ``support`` int64 [G, classes]: how many there were; ``recall`` float32
[G, classes, U] = correct / support (0 where the support is 0, never NaN); ``accuracy`` float32 [G, U] = the group's correct
over its samples; ``groups`` the G keys in order of first appearance; ``classes``; ``scores`` float64 [S, classes, U] joint
log-likelihoods and ``predictions`` uint8 [S, U], in the caller's sample order, or None."""

SVC_NMAX = 128                                  # chebgcn_searchlight_svm_query(1): the largest training set classifier='svc' serves
SVC_ITMAX = 100000                              # chebgcn_searchlight_svm_query(8): the largest max_iter
SVC_LOSSES = ('squared_hinge', 'hinge')

SolverInfo = collections.namedtuple('SolverInfo', 'sweeps residual models')
SolverInfo.__doc__ = """What ``searchlight(classifier='svc', return_solver=True)`` returns beside the result.  ``sweeps`` int32
[NM, U]: the most sweeps any class of that (model, centre) ran; ``residual`` float64 [NM, U]: the largest last-sweep ``max |PG|``
over the classes -- converged where ``residual <= tol``, ended by the cap where ``sweeps == max_iter`` and ``residual > tol``;
``models``: the ``(group key, fold)`` of every model row (``(None, fold)`` with ``within=False``)."""

_Args = collections.namedtuple('_Args', 'X tensor S M y classes indptr indices U fold gidx keys within pooled uniform vs lda shrink '
                               'svc Creg loss tol max_iter')

# The classifier keywords of ``searchlight`` and their defaults, in the order ``_check`` looks at them; the keywords every
# classifier owns; and what is said where a keyword the classifier does not own is away from its default.
_CLF_KW = dict(C=1.0, loss='squared_hinge', tol=1e-3, max_iter=1000, priors='empirical', shrinkage=0.1, variance='class',
               var_smoothing=1e-9)
_SVC_KW = ('C', 'loss', 'tol', 'max_iter')
_CLF_OWNS = {'gnb': ('priors', 'variance', 'var_smoothing'), 'lda': ('priors', 'shrinkage'), 'svc': _SVC_KW}
_SVC_ONLY = "%(who)s: C, loss, tol and max_iter belong to classifier='svc'; they mean nothing to classifier=%(clf)r"
_LDA_NONE = ("%(who)s: variance and var_smoothing mean nothing to classifier='lda' (one pooled covariance per ball, regularised by "
             "shrinkage): leave them at their defaults")
_SVC_NONE = ("%(who)s: variance, var_smoothing and shrinkage mean nothing to classifier='svc' (regularised by C): leave them at their "
             "defaults")
_NOT_OWNED = {
    'gnb': dict(dict.fromkeys(_SVC_KW, _SVC_ONLY),
                shrinkage="%(who)s: shrinkage = %(val)r means nothing to classifier='gnb' (naive Bayes has no covariance to shrink)"),
    'lda': dict(dict.fromkeys(_SVC_KW, _SVC_ONLY), variance=_LDA_NONE, var_smoothing=_LDA_NONE),
    'svc': dict(priors="%(who)s: priors = %(val)r means nothing to classifier='svc' (an SVM has no prior to set): leave it at "
                       "'empirical'", shrinkage=_SVC_NONE, variance=_SVC_NONE, var_smoothing=_SVC_NONE)}


# ---- arguments ------------------------------------------------------------------------------------------------------------------

def _neighbourhoods(nb, M, who):
    """``(indptr, indices)`` int64 of the [U, M] pattern: indices ascending, duplicates merged, values ignored."""
    if sp.issparse(nb):
        if nb.ndim != 2 or nb.shape[1] != M or nb.shape[0] < 1:
            raise ValueError('%s: neighbourhoods must be a sparse pattern [U, M = %d], got shape %r' % (who, M, tuple(nb.shape)))
        pat = sp.csr_matrix(nb, copy=True)
        pat.data = np.ones(pat.data.shape, np.int8)             # values are ignored: a stored zero is a member
    else:
        tab = nb.detach().cpu().numpy() if is_tensor(nb) else np.asarray(nb)
        if tab.ndim != 2 or tab.shape[0] != M or tab.shape[1] < 1 or tab.dtype.kind not in 'iu':
            raise ValueError('%s: neighbourhoods must be a SciPy sparse pattern [U, M] or an integer table [M = %d, k], got %s %r'
                             % (who, M, tab.dtype, tuple(tab.shape)))
        tab = tab.astype(np.int64)
        if tab.min() < 0 or tab.max() >= M:
            raise ValueError('%s: the neighbour table names vertices outside [0, %d)' % (who, M))
        rows = np.repeat(np.arange(M, dtype=np.int64), tab.shape[1] + 1)        # the centre itself is added: kNN tables leave it out
        cols = np.concatenate([np.arange(M, dtype=np.int64)[:, None], tab], axis=1).ravel()
        pat = sp.csr_matrix((np.ones(rows.size, np.int8), (rows, cols)), shape=(M, M))
    pat.sum_duplicates()
    pat.sort_indices()
    indptr, indices = pat.indptr.astype(np.int64), pat.indices.astype(np.int64)
    empty = np.flatnonzero(np.diff(indptr) == 0)
    if empty.size:
        raise ValueError('%s: neighbourhood %d is empty (%d empty rows)' % (who, empty[0], empty.size))
    return indptr, indices


def _vector(v, S, name, who):
    a = np.asarray(v.detach().cpu().numpy() if is_tensor(v) else v)
    if a.ndim != 1 or a.shape[0] != S:
        raise ValueError('%s: %s must hold one entry per sample ([S = %d]), got shape %r' % (who, name, S, a.shape))
    return a


def _patterns(samples, who):
    """``(X, tensor, S, M)`` of the ``[S, M]`` patterns, shape and dtype checked."""
    tensor = is_tensor(samples)
    X = samples if tensor else np.asarray(samples)
    if X.ndim != 2 or X.shape[0] < 2 or X.shape[1] < 1:
        raise ValueError('%s: samples must be [S >= 2, M >= 1], got shape %r' % (who, tuple(X.shape)))
    if tensor:
        if X.is_complex() or str(X.dtype) == 'torch.bool':
            raise ValueError('%s: samples of dtype %s' % (who, X.dtype))
    elif X.dtype.kind not in 'fiu':
        raise ValueError('%s: samples of dtype %s' % (who, X.dtype))
    return X, tensor, int(X.shape[0]), int(X.shape[1])


def _real(v):
    """Is ``v`` a finite real number (a bool is none)."""
    return not isinstance(v, (bool, np.bool_)) and isinstance(v, (int, float, np.integer, np.floating)) and bool(np.isfinite(v))


def _coded_labels(labels, S, classes, limits, who):
    """``(y int64 [S], classes)``: the labels as indices into ``classes`` (default: the sorted set of labels)."""
    lab = _vector(labels, S, 'labels', who)
    if lab.dtype.kind not in 'iuUSO':
        raise ValueError('%s: labels of dtype %s (ints or names)' % (who, lab.dtype))
    lab = lab.tolist()
    try:
        classes = sorted(set(lab)) if classes is None else list(classes)
        code = {c: i for i, c in enumerate(classes)}
    except TypeError:
        raise ValueError('%s: labels and classes must be sortable and hashable' % who) from None
    if len(code) != len(classes) or len(classes) < 2:
        raise ValueError('%s: at least two distinct classes are needed, got %r' % (who, classes))
    if len(classes) > (CMAX if limits else 256):
        raise ValueError('%s: %d classes; served: up to %d' % (who, len(classes), CMAX if limits else 256))
    outside = [v for v in lab if v not in code]
    if outside:
        raise ValueError('%s: label %r is not in classes %r' % (who, outside[0], classes))
    return np.array([code[v] for v in lab], np.int64), classes


def _group_keys(groups, S, who):
    """``(keys in order of first appearance, gidx int64 [S])``; ``None``: one group."""
    if is_tensor(groups) or isinstance(groups, np.ndarray):
        groups = _vector(groups, S, 'groups', who).tolist()
    _, keys, members = _runs.group_keys(groups, S, who, 'sample')
    gidx = np.empty(S, np.int64)
    for g, m in enumerate(members):
        gidx[m] = g
    return keys, gidx


def _front(samples, labels, neighbourhoods, vec, name, hint, groups, classes, batch_centres, who, limits):
    """What ``_check`` and ``_check_rdm`` share, checked in this order: the patterns, ``batch_centres``, the coded labels, the integer
    vector ``vec`` (``name``: folds or partitions), the group keys and the neighbourhoods ->
    ``(X, tensor, S, M, y, classes, vec int64, keys, gidx, indptr, indices, U)``."""
    X, tensor, S, M = _patterns(samples, who)
    if batch_centres is not None and (isinstance(batch_centres, (bool, np.bool_)) or not isinstance(batch_centres, (int, np.integer))
                                      or batch_centres < 1):
        raise ValueError('%s: batch_centres must be an int >= 1 or None, got %r' % (who, batch_centres))
    y, classes = _coded_labels(labels, S, classes, limits, who)
    vec = _vector(vec, S, name, who)
    if vec.dtype.kind not in 'iu':
        raise ValueError('%s: %s must be ints%s, got dtype %s' % (who, name, hint, vec.dtype))
    keys, gidx = _group_keys(groups, S, who)
    indptr, indices = _neighbourhoods(neighbourhoods, M, who)
    if limits and indices.size > 2 ** 31 - 1:
        raise ValueError('%s: the neighbourhoods list %d vertices; served: fewer than 2^31' % (who, indices.size))
    return X, tensor, S, M, y, classes, vec.astype(np.int64), keys, gidx, indptr, indices, int(indptr.size) - 1


def _at_default(name, val):
    """Is the classifier keyword ``name`` at its default: the default's value in the default's kind (a bool is no number, a
    float no ``max_iter``)."""
    kind = {str: str, int: (int, np.integer), float: (int, float, np.integer, np.floating)}[type(_CLF_KW[name])]
    return not isinstance(val, (bool, np.bool_)) and isinstance(val, kind) and val == _CLF_KW[name]


def _own_keyword(name, val, who):
    """Refuses a value the owner of the classifier keyword ``name`` does not serve (``variance``, ``priors`` and ``var_smoothing``
    are checked for every classifier, before this)."""
    if name == 'C' and not (_real(val) and val > 0):
        raise ValueError('%s: C must be a finite number > 0, got %r' % (who, val))
    if name == 'loss' and not (isinstance(val, str) and val in SVC_LOSSES):
        raise ValueError("%s: loss must be 'squared_hinge' or 'hinge', got %r" % (who, val))
    if name == 'tol' and not (_real(val) and val >= 0):
        raise ValueError('%s: tol must be a finite number >= 0, got %r' % (who, val))
    if name == 'max_iter' and not (_real(val) and isinstance(val, (int, np.integer)) and 1 <= val <= SVC_ITMAX):
        raise ValueError('%s: max_iter must be an int in [1, %d], got %r' % (who, SVC_ITMAX, val))
    if name == 'shrinkage' and not (isinstance(val, str) and val == 'auto') and not (_real(val) and SHRINK_MIN <= val <= 1):
        raise ValueError("%s: shrinkage must be a number in [%g, 1] or 'auto', got %r" % (who, SHRINK_MIN, val))


def _check(samples, labels, neighbourhoods, folds, groups, within, classes, scores, predictions, batch_centres, who, limits=True,
           classifier='gnb', **kw):
    """Everything that can be checked without the samples' values; ``kw``: the classifier keywords of ``_CLF_KW`` that are not at
    their defaults.  ``shrink`` of the result: the float, or -1.0 for ``'auto'``."""
    kw = dict(_CLF_KW, **kw)
    variance, priors, var_smoothing, shrinkage = (kw[k] for k in ('variance', 'priors', 'var_smoothing', 'shrinkage'))
    for name, val in (('within', within), ('scores', scores), ('predictions', predictions)):
        if not isinstance(val, (bool, np.bool_)):
            raise ValueError('%s: %s must be True or False, got %r' % (who, name, val))
    if variance not in ('class', 'pooled'):
        raise ValueError("%s: variance must be 'class' or 'pooled', got %r" % (who, variance))
    if priors not in ('empirical', 'uniform'):
        raise ValueError("%s: priors must be 'empirical' or 'uniform', got %r" % (who, priors))
    if not (_real(var_smoothing) and var_smoothing >= 0):
        raise ValueError('%s: var_smoothing must be a finite number >= 0, got %r' % (who, var_smoothing))
    if classifier not in tuple(_CLF_OWNS):
        raise ValueError("%s: classifier must be 'gnb', 'lda' or 'svc', got %r" % (who, classifier))
    for name, val in kw.items():
        if name in _CLF_OWNS[classifier]:
            _own_keyword(name, val, who)
        elif not _at_default(name, val):
            raise ValueError(_NOT_OWNED[classifier][name] % {'who': who, 'clf': classifier, 'val': val})
    X, tensor, S, M, y, classes, fold, keys, gidx, indptr, indices, U = _front(
        samples, labels, neighbourhoods, folds, 'folds', '', groups, classes, batch_centres, who, limits)
    if limits and len(keys) > GMAX:
        raise ValueError('%s: %d groups; served: up to %d' % (who, len(keys), GMAX))
    if classifier == 'lda':
        length = np.diff(indptr)
        if length.max() > LDA_PMAX:
            row = int(np.argmax(length > LDA_PMAX))
            raise ValueError("%s: neighbourhood %d holds %d vertices; classifier='lda' serves rows of up to %d (a covariance per "
                             "ball): use classifier='gnb' or, to keep the covariance, classifier='svc' for parcels and whole-brain "
                             "rows" % (who, row, length[row], LDA_PMAX))
    if scores and 8 * S * len(classes) * U > SCORES_MAX_BYTES:
        raise ValueError('%s: scores=True would return %d bytes ([S, classes, U] float64); refused beyond %d: score fewer centres '
                         'per call' % (who, 8 * S * len(classes) * U, SCORES_MAX_BYTES))
    # a class without a training sample, in a training set that has test samples
    fvals, fidx = np.unique(fold, return_inverse=True)
    cnt = np.zeros((len(keys), fvals.size, len(classes)), np.int64)
    np.add.at(cnt, (gidx, fidx, y), 1)
    if not within:
        cnt = cnt.sum(axis=0, keepdims=True)
    train = cnt.sum(axis=1, keepdims=True) - cnt                # [G or 1, F, C]: the training samples of the model tested on (g, f)
    bad = np.argwhere((train == 0) & (cnt.sum(axis=2, keepdims=True) > 0))
    if bad.size:
        g, f, c = (int(v) for v in bad[0])
        raise ValueError('%s: class %r has no training sample for the test samples of %sfold %d' % (
            who, classes[c], 'group %r, ' % (keys[g],) if within else '', int(fvals[f])))
    if classifier == 'svc':
        size = train.sum(axis=2)                                # [G or 1, F]: the samples of the training set tested on (g, f)
        big = np.argwhere((size > SVC_NMAX) & (cnt.sum(axis=2) > 0))
        if big.size:
            g, f = (int(v) for v in big[0])
            raise ValueError("%s: the training set of %sfold %d holds %d samples; classifier='svc' serves up to %d (the Gram matrix "
                             "of the training samples stays on chip); across-subject training sets of thousands of samples are out "
                             "of scope, so within=False is served only while n <= %d"
                             % (who, 'group %r, ' % (keys[g],) if within else '', int(fvals[f]), size[g, f], SVC_NMAX, SVC_NMAX))
    return _Args(X, tensor, S, M, y, classes, indptr, indices, U, fold, gidx, keys, bool(within), variance == 'pooled', priors == 'uniform',
                 float(var_smoothing), classifier == 'lda', -1.0 if isinstance(shrinkage, str) else float(shrinkage),
                 classifier == 'svc', float(kw['C']), kw['loss'], float(kw['tol']), int(kw['max_iter']))


def _summary(correct, support, xp):
    """``(recall, accuracy)`` float32 from the counts: float64 quotients rounded once."""
    if xp is np:
        s = support.astype(np.float64)
        recall = (correct / np.where(s > 0, s, 1.0)[:, :, None]).astype(np.float32)
        accuracy = (correct.sum(axis=1) / np.maximum(s.sum(axis=1), 1.0)[:, None]).astype(np.float32)
        return recall, accuracy
    s = support.to(xp.float64)
    recall = (correct.to(xp.float64) / xp.where(s > 0, s, xp.ones_like(s))[:, :, None]).to(xp.float32)
    accuracy = (correct.sum(dim=1).to(xp.float64) / xp.clamp(s.sum(dim=1), min=1.0)[:, None]).to(xp.float32)
    return recall, accuracy


def _support(a):
    support = np.zeros((len(a.keys), len(a.classes)), np.int64)
    np.add.at(support, (a.gidx, a.y), 1)
    return support


# ---- the host restatement -------------------------------------------------------------------------------------------------------

def searchlight_host(samples, labels, neighbourhoods, folds, groups=None, within=True, classes=None, variance='class',
                     priors='empirical', var_smoothing=1e-9, scores=False, predictions=False, device=None, batch_centres=None,
                     return_scale=False, classifier='gnb', shrinkage=0.1, C=1.0, loss='squared_hinge', tol=1e-3, max_iter=1000,
                     return_solver=False):
    """``searchlight`` restated in float64 NumPy (no device; ``device`` and ``batch_centres`` are accepted and ignored), the
    obvious way: per training set and per centre the ball's columns are sliced out, the class means and variances fitted on
    them (``sum / n``, ``sum (x - mean)^2 / n``), every test sample scored with
    ``log prior - sum_v [(x - mu)^2 / (2 var) + log(2 pi var) / 2]`` and the first maximal class taken.  The samples are rounded to
    float32 first, as staging does.  Returns a ``SearchlightResult`` of NumPy arrays; with ``return_scale`` a pair of it and
    ``scale`` float64 [S, classes, U] ``= |log prior| + sum_v [(x - mu)^2 / (2 var) + |log(2 pi var) / 2|]``, the magnitude an
    error bound of a score is stated in.

    ``classifier='lda'``: the model of ``searchlight``'s docstring, per training set and per centre: the ball's columns sliced
    out, the residuals formed with NumPy, ``scipy.linalg.cho_factor`` / ``cho_solve``, the scores.  There ``scale`` is
    ``kappa (|log prior_c| + |d_c . w_c| / 2 + sum_v |w_cv| |x_sv - m_v|)``, ``kappa`` the 2-norm condition number of that
    (model, centre)'s ``Sigma`` (``eigvalsh``; 1 in the degenerate case): the magnitude a float64 solve may be off by.

    ``classifier='svc'``: the model of ``searchlight``'s docstring with its chains as explicit loops over samples and vertices,
    vectorised across (i, j) and across the classes; every operation a separate correctly rounded one, so the device agrees
    with it bit for bit.  ``return_solver``: a pair of the result and a ``SolverInfo`` (``return_scale`` is not served there)."""
    who = 'searchlight_host'
    a = _check(samples, labels, neighbourhoods, folds, groups, within, classes, scores, predictions, batch_centres, who, limits=False,
               classifier=classifier, variance=variance, priors=priors, var_smoothing=var_smoothing, shrinkage=shrinkage, C=C,
               loss=loss, tol=tol, max_iter=max_iter)
    _solver_flag(return_solver, a, who)
    if a.svc and return_scale:
        raise ValueError("%s: return_scale is not served with classifier='svc' (the device agrees bit for bit)" % who)
    X = host_array(a.X, who).astype(np.float64)
    S, C, U, G = a.S, len(a.classes), a.U, len(a.keys)
    sc = np.empty((S, C, U))
    scale = np.empty((S, C, U)) if return_scale else None
    pred = np.empty((S, U), np.uint8)
    key = a.gidx * (int(a.fold.max()) - int(a.fold.min()) + 1) + (a.fold - a.fold.min()) if a.within else a.fold
    model_keys = np.unique(key)
    sweeps, residual, models = np.zeros((model_keys.size, U), np.int32), np.zeros((model_keys.size, U)), []
    ball = _svc_host_ball if a.svc else _lda_host_ball if a.lda else _gnb_host_ball
    for mi, k in enumerate(model_keys):
        test = key == k
        train = ~test & (a.gidx == a.gidx[test][0]) if a.within else ~test
        Xtr, ytr, Xte = X[train], a.y[train], X[test]
        models.append((a.keys[a.gidx[test][0]] if a.within else None, int(a.fold[test][0])))
        n = np.array([(ytr == c).sum() for c in range(C)], np.float64)
        logp = np.full(C, -np.log(C)) if a.uniform else np.log(n / n.sum())
        eps = a.vs * Xtr.var(axis=0).max()
        for u in range(U):
            cols = a.indices[a.indptr[u]:a.indptr[u + 1]]
            s_, q_, sweeps[mi, u], residual[mi, u] = ball(Xtr[:, cols], ytr, Xte[:, cols], n, logp, eps, a)
            sc[test, :, u] = s_
            if return_scale:
                scale[test, :, u] = q_
            pred[test, u] = np.argmax(s_, axis=1)
    correct = np.zeros((G, C, U), np.int32)
    np.add.at(correct, (a.gidx[:, None], a.y[:, None], np.arange(U)[None, :]), (pred == a.y[:, None]).astype(np.int32))
    support = _support(a)
    recall, accuracy = _summary(correct, support, np)
    res = SearchlightResult(correct, support, recall, accuracy, list(a.keys), list(a.classes), sc if scores else None,
                            pred if predictions else None)
    if return_solver:
        return res, SolverInfo(sweeps, residual, models)
    return (res, scale) if return_scale else res


def _solver_flag(return_solver, a, who):
    if not isinstance(return_solver, (bool, np.bool_)):
        raise ValueError('%s: return_solver must be True or False, got %r' % (who, return_solver))
    if return_solver and not a.svc:
        raise ValueError("%s: return_solver belongs to classifier='svc' (the other classifiers have no iteration to report)" % who)


# The classifier of one (training set, row): ``A`` [n, P] training columns in list order with labels ``ytr``, ``T`` [t, P] test
# columns, class counts ``n`` and log priors ``logp`` [C], the smoothing ``eps`` -> ``(scores, scale or None [t, C], sweeps, residual)``.

def _gnb_host_ball(A, ytr, T, n, logp, eps, a):
    """Gaussian naive Bayes: ``sum / n``, ``sum (x - mean)^2 / n``, the joint log-likelihoods."""
    C = n.size
    mu = np.stack([A[ytr == c].sum(axis=0) / n[c] for c in range(C)])
    ss = np.stack([((A[ytr == c] - mu[c]) ** 2).sum(axis=0) for c in range(C)])
    var = (np.broadcast_to(ss.sum(axis=0) / n.sum(), ss.shape) if a.pooled else ss / n[:, None]) + eps
    ok = var > 0                                                # a vertex whose smoothed variance is 0 contributes nothing
    v = np.where(ok, var, 1.0)
    scores, scale = np.empty((T.shape[0], C)), np.empty((T.shape[0], C))
    for c in range(C):
        q = np.where(ok[c], (T - mu[c]) ** 2 / (2.0 * v[c]), 0.0)
        lg = np.where(ok[c], 0.5 * np.log(2.0 * np.pi * v[c]), 0.0)
        scores[:, c] = logp[c] - (q + lg).sum(axis=1)
        scale[:, c] = abs(logp[c]) + (q + np.abs(lg)).sum(axis=1)
    return scores, scale, 0, 0.0


def _svc_host_ball(A, ytr, T, n, logp, eps, a):
    """The one-vs-rest linear SVM: the model of ``searchlight``'s docstring, operation by operation; no scale."""
    C, Creg, loss, tol, max_iter = n.size, a.Creg, a.loss, a.tol, a.max_iter
    n, P = A.shape
    acc = np.zeros(P)
    for k in range(n):                                          # m_v: one chain in list order, one division
        acc = acc + A[k]
    m = acc / float(n)
    Ac, Tc = A - m, T - m
    K, Kt = np.zeros((n, n)), np.zeros((T.shape[0], n))
    for v in range(P):                                          # K_ij: one chain over the vertices per element
        K = K + Ac[:, v, None] * Ac[None, :, v]
        Kt = Kt + Tc[:, v, None] * Ac[None, :, v]
    q = K + 1.0
    D, Ub = (1.0 / (2.0 * Creg), np.inf) if loss == 'squared_hinge' else (0.0, Creg)
    Qd = np.diagonal(q) + D
    t = np.where(ytr[None, :] == np.arange(C)[:, None], 1.0, -1.0)              # [C, n]
    alpha, g = np.zeros((C, n)), np.full((C, n), -1.0)
    live = np.ones(C, bool)
    sweeps, resid = np.zeros(C, np.int32), np.zeros(C)
    for e in range(1, max_iter + 1):
        mx = np.zeros(C)
        for i in range(n):
            G, ai = g[:, i].copy(), alpha[:, i].copy()
            PG = np.where(ai == 0.0, np.minimum(G, 0.0), np.where(ai == Ub, np.maximum(G, 0.0), G))
            act = live & (PG != 0.0)
            if act.any():
                an = np.minimum(np.maximum(ai[act] - G[act] / Qd[i], 0.0), Ub)
                delta = an - ai[act]
                g[act] = g[act] + (t[act, i, None] * t[act]) * (delta[:, None] * q[None, :, i])
                g[act, i] = g[act, i] + delta * D
                alpha[act, i] = an
            mx = np.maximum(mx, np.abs(PG))
        sweeps[live], resid[live] = e, mx[live]
        live &= ~(mx <= tol)
        if not live.any():
            break
    at = alpha * t
    f = np.zeros((T.shape[0], C))
    for j in range(n):                                          # the score: one chain in list order
        f = f + at[None, :, j] * (Kt[:, j, None] + 1.0)
    return f, None, int(sweeps.max()), float(resid.max())


def lda_shrinkage_host(R):
    """The Ledoit-Wolf shrinkage of ``classifier='lda'`` with ``shrinkage='auto'``, on a matrix ``R`` [n, P] of class-centred
    residuals (float64): with ``S = R.T R / n`` and ``nu = tr S / P``,  ``beta_ = sum_k (sum_i r_ki^2)^2``,
    ``delta_ = sum_ij S_ij^2``, ``beta = (beta_ / n - delta_) / (P n)``, ``delta = (delta_ - 2 nu tr S + P nu^2) / P``,
    ``beta = min(beta, delta)``, ``g = beta / delta`` (0 where ``beta == 0``), clipped into ``[SHRINK_MIN, 1]`` --
    ``sklearn.covariance.ledoit_wolf(R, assume_centered=True)[1]`` above the floor."""
    R = np.asarray(R, np.float64)
    if R.ndim != 2 or R.shape[0] < 1 or R.shape[1] < 1:
        raise ValueError('lda_shrinkage_host: R must be [n >= 1, P >= 1], got shape %r' % (R.shape,))
    n, P = R.shape
    S = R.T @ R / n
    tr = np.trace(S)
    nu = tr / P
    beta_ = float((((R ** 2).sum(axis=1)) ** 2).sum())
    delta_ = float((S ** 2).sum())
    beta = (beta_ / n - delta_) / (P * n)
    delta = (delta_ - 2.0 * nu * tr + P * nu ** 2) / P
    beta = min(beta, delta)
    g = 0.0 if beta == 0 else beta / delta
    return float(min(max(g, SHRINK_MIN), 1.0))


def _lda_host_ball(A, ytr, T, n, logp, eps, a):
    """Shrinkage LDA: ``scipy.linalg.cho_factor`` / ``cho_solve`` on the shrunk pooled covariance of the ball."""
    import scipy.linalg
    shrink = a.shrink
    C, P = n.size, A.shape[1]
    order = np.concatenate([np.flatnonzero(ytr == c) for c in range(C)])        # class 0's samples first, as the plan lists them
    mu = np.stack([A[ytr == c].sum(axis=0) / n[c] for c in range(C)])
    m = (n[:, None] * mu).sum(axis=0) / n.sum()
    d = mu - m
    R = (A - mu[ytr])[order]
    S = R.T @ R / n.sum()
    tr = np.trace(S)
    nu = tr / P
    g = lda_shrinkage_host(R) if shrink < 0 else shrink
    w, kappa = np.zeros((C, P)), 1.0
    if tr > 0:
        Sigma = (1.0 - g) * S + g * nu * np.eye(P)
        try:
            w = scipy.linalg.cho_solve(scipy.linalg.cho_factor(Sigma, lower=True), d.T).T
            ev = np.linalg.eigvalsh(Sigma)
            kappa = float(ev[-1] / ev[0])
        except np.linalg.LinAlgError:
            w = np.zeros((C, P))
        if not (np.isfinite(w).all() and np.isfinite(kappa) and kappa > 0):
            w, kappa = np.zeros((C, P)), 1.0
    dw = (d * w).sum(axis=1)
    Tc = T - m
    scores = logp - 0.5 * dw + Tc @ w.T
    scale = kappa * (np.abs(logp) + 0.5 * np.abs(dw) + np.abs(Tc) @ np.abs(w).T)
    return scores, scale, 0, 0.0


# ---- the device -----------------------------------------------------------------------------------------------------------------

_Plan = collections.namedtuple('_Plan', 'order test_ptr tmax list_ptr list_idx class_ptr class_idx logprior sgroup slabel NM NC')


def _device_plan(a, NC):
    """The tables of the kernels: the samples sorted by model (stable, so the test samples of a model are contiguous and keep
    the caller's order), and per model its training samples in the caller's ascending order, as positions in the sorted order."""
    C = len(a.classes)
    _, fidx = np.unique(a.fold, return_inverse=True)
    model = (a.gidx * (int(fidx.max()) + 1) + fidx) if a.within else fidx
    ids, model = np.unique(model, return_inverse=True)
    NM = int(ids.size)
    order = np.argsort(model, kind='stable')
    pos = np.empty(a.S, np.int64)
    pos[order] = np.arange(a.S)
    counts = np.bincount(model, minlength=NM)
    test_ptr = np.concatenate([[0], np.cumsum(counts)])
    first = order[test_ptr[:-1]]                                # one test sample of every model
    lists, clists = [], []
    logprior = np.zeros((NM, NC))
    for m in range(NM):
        train = model != m
        if a.within:
            train &= a.gidx == a.gidx[first[m]]
        train = np.flatnonzero(train)
        lists.append(pos[train])
        per = [pos[train[a.y[train] == c]] for c in range(C)]
        clists += per
        n = np.array([p.size for p in per], np.float64)
        logprior[m, :C] = -np.log(C) if a.uniform else np.log(n / n.sum())
    ptr = lambda ls: np.concatenate([[0], np.cumsum([l.size for l in ls])]).astype(np.int32)
    if sum(l.size for l in lists) > 2 ** 31 - 1:
        raise ValueError('searchlight: %d models over %d samples list more than 2^31 training samples' % (NM, a.S))
    i32 = lambda v: np.ascontiguousarray(v, np.int32)
    return _Plan(order, i32(test_ptr), int(counts.max()), ptr(lists), i32(np.concatenate(lists)), ptr(clists),
                 i32(np.concatenate(clists)), logprior, i32(a.gidx[order]), i32(a.y[order]), NM, NC)


def _transposed(X, order, dev):
    """``Xt`` float32 [M, plane_stride(S)]: the patterns vertex-major, samples in the plan's order (torch plumbing)."""
    import torch
    from . import _lib
    S, M = X.shape
    Xt = torch.zeros((M, _lib.plane_stride(S)), dtype=torch.float32, device=dev)
    Xt[:, :S] = X[torch.as_tensor(order).to(dev)].t()
    return Xt


def _outputs(a, dev, scores, predictions):
    """``(correct int32 [G, C, U] of zeros, scores float64 [S, C, U] or None, predictions uint8 [S, U] or None)`` on ``dev``."""
    import torch
    S, C, U = a.S, len(a.classes), a.U
    return (torch.zeros((len(a.keys), C, U), dtype=torch.int32, device=dev),
            torch.empty((S, C, U), dtype=torch.float64, device=dev) if scores else None,
            torch.empty((S, U), dtype=torch.uint8, device=dev) if predictions else None)


def _upload(a, plan, dev, names):
    """The CSR rows of the neighbourhoods (``rowptr``, ``colidx``, int32) and the tables ``names`` of the plan on ``dev``, each
    uploaded once; ``order`` goes as int32 (the kernels' ``sorig``)."""
    import torch
    up = lambda v: torch.as_tensor(v).to(dev)
    tables = {name: up(plan.order.astype(np.int32) if name == 'order' else getattr(plan, name)) for name in names.split()}
    return types.SimpleNamespace(rowptr=up(a.indptr.astype(np.int32)), colidx=up(a.indices.astype(np.int32)), **tables)


def _row_batches(a, buckets, batch_centres, dev):
    """``(bucket, rows int32 on dev)``: the centres bucket by bucket of row length (``buckets``: the bucket of every length), and
    inside a bucket batch by batch of ``batch_centres`` (``None``: the whole bucket)."""
    import torch
    of_row = np.array([buckets[int(n)] for n in np.diff(a.indptr)])
    for bucket in sorted(set(of_row.tolist())):
        rows = np.flatnonzero(of_row == bucket).astype(np.int32)
        step = rows.size if batch_centres is None else int(min(batch_centres, rows.size))
        for i in range(0, rows.size, step):
            yield bucket, torch.as_tensor(rows[i:i + step]).to(dev)


def _run(a, plan, Xt, scores, predictions, batch_centres):
    """The launches, on the current device: spread, fit, then the centres batch by batch.  Returns device tensors."""
    from . import ops
    t = _upload(a, plan, Xt.device, 'list_ptr list_idx class_ptr class_idx test_ptr logprior sgroup slabel order')
    S, C, U = a.S, len(a.classes), a.U
    spread = ops.searchlight_spread(Xt, S, t.list_ptr, t.list_idx)
    eps = a.vs * spread.max(dim=1).values
    par, lg = ops.searchlight_fit(Xt, S, t.class_ptr, t.class_idx, C, eps, pooled=a.pooled)
    correct, sc, pred = _outputs(a, Xt.device, scores, predictions)
    if batch_centres is None:
        batch_centres = max(1, (64 << 20) // (8 * plan.NM * plan.NC))           # 64 MiB of per-centre offsets per launch
    batch_centres = int(min(batch_centres, U, (2 ** 31 - 1) // CMAX))
    for u0 in range(0, U, batch_centres):
        ops.searchlight_score(Xt, S, t.rowptr, t.colidx, u0, min(batch_centres, U - u0), t.test_ptr, plan.tmax, C, par, lg, t.logprior,
                              t.sgroup, t.slabel, t.order, correct, scores=sc, predictions=pred)
    return correct, sc, pred


def _run_lda(a, plan, Xt, scores, predictions, batch_centres, gamma=False):
    """The launches of ``classifier='lda'``: fit (``eps = 0``: only its means are used), then the centres bucket by bucket of row
    length and batch by batch.  Returns device tensors; with ``gamma`` a fourth, float64 [NM, U]: the shrinkage used."""
    import torch
    from . import ops
    dev = Xt.device
    t = _upload(a, plan, dev, 'class_ptr class_idx test_ptr logprior sgroup slabel order')
    S, C = a.S, len(a.classes)
    par, _ = ops.searchlight_fit(Xt, S, t.class_ptr, t.class_idx, C, torch.zeros(plan.NM, dtype=torch.float64, device=dev))
    correct, sc, pred = _outputs(a, dev, scores, predictions)
    gam = torch.empty((plan.NM, a.U), dtype=torch.float64, device=dev) if gamma else None
    for bucket, rows in _row_batches(a, ops.searchlight_lda_geometry()['buckets'], batch_centres, dev):
        ops.searchlight_lda(Xt, S, t.rowptr, t.colidx, rows, bucket, t.class_ptr, t.class_idx, t.test_ptr, plan.tmax, C, par,
                            t.logprior, a.shrink, t.sgroup, t.slabel, t.order, correct, scores=sc, predictions=pred, gamma_out=gam)
    return (correct, sc, pred, gam) if gamma else (correct, sc, pred)


def _run_svc(a, plan, Xt, scores, predictions, batch_centres):
    """The launches of ``classifier='svc'``: the models bucket by bucket of training-set size, the centres batch by batch (ranges
    of consecutive centres, every one against every model of the bucket: not the rows of ``_row_batches``).  Returns device
    tensors: ``(correct, scores, predictions, sweeps int32 [NM, U], residual float64 [NM, U])``."""
    import torch
    from . import ops
    dev = Xt.device
    up = lambda v: torch.as_tensor(v).to(dev)
    t = _upload(a, plan, dev, 'list_ptr list_idx test_ptr sgroup slabel order')
    S, C, U = a.S, len(a.classes), a.U
    correct, sc, pred = _outputs(a, dev, scores, predictions)
    sweeps = torch.zeros((plan.NM, U), dtype=torch.int32, device=dev)
    residual = torch.zeros((plan.NM, U), dtype=torch.float64, device=dev)
    buckets = ops.searchlight_svm_geometry()['buckets']
    of_model = np.array([buckets[int(n)] for n in np.diff(plan.list_ptr)])
    step = U if batch_centres is None else int(min(batch_centres, U))
    for bucket in sorted(set(of_model.tolist())):
        models = up(np.flatnonzero(of_model == bucket).astype(np.int32))
        for u0 in range(0, U, step):
            ops.searchlight_svm(Xt, S, t.rowptr, t.colidx, up(np.arange(u0, min(u0 + step, U), dtype=np.int32)), models, bucket,
                                t.list_ptr, t.list_idx, t.test_ptr, plan.tmax, C, a.Creg, a.loss, a.tol, a.max_iter, t.sgroup,
                                t.slabel, t.order, correct, scores=sc, predictions=pred, sweeps=sweeps, residual=residual)
    return correct, sc, pred, sweeps, residual


def _result(a, correct, sc, pred, as_tensor):
    import torch
    support = _support(a)
    if as_tensor:
        recall, accuracy = _summary(correct, torch.as_tensor(support).to(correct.device), torch)
        return SearchlightResult(correct, support, recall, accuracy, list(a.keys), list(a.classes), sc, pred)
    correct = correct.cpu().numpy()
    recall, accuracy = _summary(correct, support, np)
    return SearchlightResult(correct, support, recall, accuracy, list(a.keys), list(a.classes),
                             None if sc is None else sc.cpu().numpy(), None if pred is None else pred.cpu().numpy())


def _staged(a, order, dev, who):
    """``_transposed`` of the checked patterns on ``dev``, samples in ``order``; a tensor's values are checked here."""
    import torch
    if a.tensor:
        X = a.X.detach().to(dev, torch.float32)
        if not bool(torch.isfinite(X).all()):
            raise ValueError('%s: samples hold non-finite values' % who)
    else:
        X = torch.as_tensor(a.X).to(dev)                        # (float32 and finite: the caller's host_array)
    return _transposed(X, order, dev)


def _searchlight(a, dev, scores, predictions, batch_centres, as_tensor, who, return_solver=False):
    import torch
    from . import ops
    NC = ops.searchlight_geometry()['buckets'][len(a.classes)]
    plan = _device_plan(a, NC)
    if plan.NM > NMAX:
        raise ValueError('%s: %d training sets; served: up to %d' % (who, plan.NM, NMAX))
    with torch.cuda.device(dev):
        Xt = _staged(a, plan.order, dev, who)
        if a.svc:
            correct, sc, pred, sweeps, residual = _run_svc(a, plan, Xt, scores, predictions, batch_centres)
            res = _result(a, correct, sc, pred, as_tensor)
            if not return_solver:
                return res
            first = plan.order[plan.test_ptr[:-1]]              # one test sample of every model
            models = [(a.keys[a.gidx[s]] if a.within else None, int(a.fold[s])) for s in first]
            if not as_tensor:
                sweeps, residual = sweeps.cpu().numpy(), residual.cpu().numpy()
            return res, SolverInfo(sweeps, residual, models)
        correct, sc, pred = (_run_lda if a.lda else _run)(a, plan, Xt, scores, predictions, batch_centres)
        return _result(a, correct, sc, pred, as_tensor)


def searchlight(samples, labels, neighbourhoods, folds, groups=None, within=True, classes=None, variance='class', priors='empirical',
                var_smoothing=1e-9, scores=False, predictions=False, device=None, batch_centres=None, classifier='gnb', shrinkage=0.1,
                C=1.0, loss='squared_hinge', tol=1e-3, max_iter=1000, return_solver=False):
    """Cross-validated accuracy of a Gaussian naive-Bayes (``classifier='gnb'``), a shrinkage-LDA (``'lda'``) or a linear-SVM
    (``'svc'``) classifier at every centre, on the device: a ``SearchlightResult``.

    ``samples``: ``[S, M]`` patterns, one per trial (trial means, betas); NumPy or a torch tensor; rounded to float32 as staging
    does.  ``labels``: ``[S]`` values found in ``classes``, which defaults to the sorted set of labels (the order of
    ``EventWindows.classes``).  ``neighbourhoods``: a SciPy sparse pattern ``[U, M]`` whose row u lists the vertices centre u
    sees -- ``graph.hop_balls(A, 2)`` for the searchlight map, one row per parcel for ROI decoding, one full row for the
    whole-brain baseline; values are ignored, indices are sorted ascending and duplicates merged, nothing is added.  An
    ``[M, k]`` integer table such as ``knn_device`` returns is accepted too, and there the centre itself IS added to its row
    (such tables leave it out).  ``folds``: ``[S]`` ints; a sample is tested by the model fitted without its fold.
    ``groups``: ``[S]`` hashable keys -- the subject; default one group.  ``within=True``: the model for a test sample of
    (group g, fold f) is fitted on the samples of g with fold != f (within-subject leave-one-run-out); ``within=False``: on all
    samples with fold != f (across subjects: keep a subject in one fold, e.g. with ``splits.subject_folds``).  Either way the
    counts are reported per group.

    The model, per (training set, class c, vertex v), in float64: ``mu = sum x / n``, ``var = sum (x - mu)^2 / n`` in two
    passes over the class's training samples in ascending sample order; ``variance='pooled'`` replaces it by
    ``sum_c sum (x - mu_c)^2 / sum_c n_c`` (diagonal LDA).  Every variance gets ``eps = var_smoothing * max over ALL M vertices
    of the variance of the whole training set`` added -- scikit-learn's ``GaussianNB`` rule, but with the maximum taken over
    the whole brain instead of over the ball, so that the parameter tables stay per vertex and one fit serves every centre (on
    a row of all vertices the two coincide); a vertex whose smoothed variance is 0 contributes nothing.  ``priors``: the class
    frequencies of the training set (``'empirical'``) or ``'uniform'``.
    ``score[s, c, u] = log prior_c - sum_{v in row u, ascending} [(x_sv - mu_cv)^2 / (2 var_cv) + log(2 pi var_cv) / 2]``; the
    prediction is the first maximal class.

    ``classifier='lda'``: a full covariance inside the ball, for rows of up to ``LDA_PMAX`` = 128 vertices; ``variance`` and
    ``var_smoothing`` must stay at their defaults.  Per (training set, centre with vertices ``v_0 < ... < v_{P-1}``), in float64:
    ``n_c`` the training samples of class c, ``n = sum n_c``; ``mu_cv`` the class means as above; ``m_v = (sum_c n_c mu_cv) / n``;
    ``d_cv = mu_cv - m_v``; the pooled within-class covariance ``S_ij = (sum_k r_ki r_kj) / n`` over the training samples (class 0's
    first, each class in ascending sample order), ``r_kv = x_kv - mu_{y_k, v}``; ``nu = tr S / P``;
    ``Sigma = (1 - g) S + g nu I``; ``w_c = Sigma^-1 d_c`` by Cholesky; ``b_c = log prior_c - d_c . w_c / 2``;
    ``score[s, c, u] = b_c + sum_v w_cv (x_sv - m_v)``; the prediction is the first maximal class.  Up to a term common to all
    classes this is scikit-learn's ``LinearDiscriminantAnalysis(solver='lsqr', shrinkage=g).decision_function``.  As there, the
    covariance is weighted by the empirical class frequencies whatever ``priors`` says: ``priors`` changes the intercept only.
    ``shrinkage``: ``g``, a number in ``[SHRINK_MIN, 1]`` = [1e-6, 1], or ``'auto'``: the Ledoit-Wolf coefficient of the residuals
    (``lda_shrinkage_host``), clipped into that range.  The floor keeps ``Sigma`` positive definite with a condition number of at
    most about ``P / g`` -- with fewer training samples than vertices ``S`` is singular, which is the normal case -- so no
    pivoting and no borderline decision is needed.  If ``tr S`` is not > 0 (every vertex of the ball constant within every
    class) or a Cholesky pivot is not positive and finite, ``w = 0`` and ``b_c = log prior_c``: the prior decides, nothing is NaN.
    ``scores`` are then discriminant values, not log-likelihoods.  With ``'gnb'`` ``shrinkage`` must stay at its default.

    ``classifier='svc'``: a one-vs-rest linear SVM in its dual form, for rows of ANY length and training sets of up to
    ``SVC_NMAX`` = 128 samples; ``priors``, ``variance``, ``var_smoothing`` and ``shrinkage`` must stay at their defaults (an SVM
    has no prior to set).  Float64 throughout, and every operation is a separate correctly rounded multiply, add or divide --
    nothing is fused -- so ``searchlight_host`` agrees bit for bit.  Per training set with samples ``k_0 < ... < k_{n-1}`` and per
    row with vertices ``v_0 < ... < v_{P-1}``, P >= 1:  centring ``m_v = (x_{k_0 v} + x_{k_1 v} + ...) / n``, one chain in that
    order, then one division;  Gram matrix ``K_ij = sum_v (x_iv - m_v)(x_jv - m_v)``, one chain over the vertices in ascending
    order, for the training pairs and every (test sample, training sample) pair;  one-vs-rest with liblinear's regularised bias
    (``fit_intercept=True, intercept_scaling=1``: the kernel is ``K + 1``): for class c  ``t_i = +1`` if ``y_i = c`` else ``-1``,
    ``q_ij = K_ij + 1``, ``Q_ij = t_i t_j q_ij``;  ``loss='hinge'``: ``D = 0``, upper bound ``Ub = C``;  ``loss='squared_hinge'``:
    ``D = 1 / (2 C)``, no upper bound;  ``Qd_i = q_ii + D`` (>= 1: no division needs a guard, there is no degenerate branch).
    Dual coordinate descent (Hsieh et al. 2008) in fixed cyclic order, no shuffling, no shrinking of the active set:
    ``alpha = 0``, ``g_i = -1``; sweeps e = 1 .. ``max_iter``, each visiting i = 0 .. n - 1:  ``G = g_i``;  ``PG = min(G, 0)`` if
    ``alpha_i == 0``, ``max(G, 0)`` if ``alpha_i == Ub``, else ``G``;  if ``PG != 0``:  ``a = min(max(alpha_i - G / Qd_i, 0), Ub)``,
    ``delta = a - alpha_i``, ``alpha_i = a``, for every j ``g_j = g_j + (t_i t_j)(delta q_ji)`` and at j = i additionally, as a
    second addition, ``g_i = g_i + delta D``;  after a sweep, stop if the sweep's ``max |PG| <= tol``.
    ``score[s, c, u] = sum_j (alpha_j t_j)(K_sj + 1)``, one chain in list order; the prediction is the first maximal class.  For
    two classes the problems are mirror images and ``score[:, 1] == -score[:, 0]`` exactly.  At convergence this is
    scikit-learn's ``LinearSVC(loss=, C=, dual=True, fit_intercept=True, intercept_scaling=1, multi_class='ovr')`` on the row's
    columns centred by the training means; the primal is strongly convex in (w, b), so the decision values are unique.  Scaling
    the patterns is the caller's job, and ``C`` is on the data's scale.  ``C``: finite, > 0; ``loss``: ``'squared_hinge'``
    (scikit-learn's default) or ``'hinge'``; ``tol``: finite, >= 0; ``max_iter``: an int in [1, 100000].  Where n is much larger
    than P and ``C >= 1`` the descent needs thousands of sweeps and the cap ends it: ``return_solver=True`` returns
    ``(result, SolverInfo)`` with the sweeps run and the last sweep's ``max |PG|`` of every (model, centre), so that convergence
    is reported and never hidden.  With the other classifiers these keywords must stay at their defaults.

    ``scores`` / ``predictions``: also return the float64 ``[S, classes, U]`` scores (refused beyond 2 GiB) / the uint8
    ``[S, U]`` predictions.  ``batch_centres``: centres of one launch; the result does not depend on it, bit for bit.  The
    maps are NumPy arrays, or device tensors if ``samples`` came as a tensor.  Group inference on the maps:
    ``map_test(res.recall - 1 / len(res.classes), A)``.

    ``ValueError`` before any launch: malformed shapes and dtypes, non-finite samples, fewer than two classes or more than 32,
    a label outside ``classes``, an empty neighbourhood, ``var_smoothing < 0``, unknown strings, a class without a training
    sample in a training set that has test samples (naming the group and the fold); with ``'lda'`` a row of more than 128
    vertices (naming it), a ``shrinkage`` outside ``[1e-6, 1]`` that is not ``'auto'``, ``variance`` or ``var_smoothing`` away from
    their defaults; with ``'gnb'`` a ``shrinkage`` away from its default; with ``'svc'`` a training set of more than 128 samples
    (naming the group, the fold and the count: across-subject training sets of thousands of samples are out of scope, so
    ``within=False`` is served only while n <= 128), a bad ``C``, ``loss``, ``tol`` or ``max_iter``, ``priors='uniform'``,
    ``variance``, ``var_smoothing`` or ``shrinkage`` away from their defaults; without ``'svc'`` its keywords away from theirs.

    Out of scope: SVM training sets above 128 samples (a Gram matrix in HBM), non-linear kernels, one-vs-one or Crammer-Singer
    multi-class, an unregularised bias (libsvm's equality constraint), class weights, per-class covariances (QDA), ``'lda'`` on
    balls above 128 vertices, returning the discriminant or primal weights, label-permutation nulls per subject (group inference
    goes through ``map_test``), smoothing per ball, temporal features beyond the trial mean, any scaling or cleaning of the
    patterns or the series."""
    who = 'searchlight'
    a = _check(samples, labels, neighbourhoods, folds, groups, within, classes, scores, predictions, batch_centres, who,
               classifier=classifier, variance=variance, priors=priors, var_smoothing=var_smoothing, shrinkage=shrinkage, C=C,
               loss=loss, tol=tol, max_iter=max_iter)
    _solver_flag(return_solver, a, who)
    if not a.tensor:
        a = a._replace(X=host_array(a.X, who))                  # non-finite values: before the device is touched
    return _searchlight(a, _runs.cuda_device(device, a.X), scores, predictions, batch_centres, a.tensor, who,
                        bool(return_solver))


# ---- from event designs ---------------------------------------------------------------------------------------------------------

_MATCH_KW = ('start_trial', 'hrf_delay', 'flag_event', 'rest')


def default_folds(groups, within=True):
    """The folds ``searchlight_events`` gives runs by default, one per run: the run's position among the runs of its group
    (``within``: leave-one-run-out inside every subject), or its group's index in order of first appearance (leave one subject
    out)."""
    seen = {}
    out = []
    for g in groups:
        if g not in seen:
            seen[g] = [len(seen), 0]
        out.append(seen[g][1] if within else seen[g][0])
        seen[g][1] += 1
    return np.array(out, np.int64)


def _events_plan(lengths, label_runs, target_name, block_dura, groups, folds, within, match_kw, who='searchlight_events'):
    """The host part of ``searchlight_events``: ``(idx int64 [S, block_dura] rows of the concatenated runs, labels, groups and
    folds per trial, classes)``."""
    from . import events
    R = len(lengths)
    if isinstance(block_dura, (bool, np.bool_)) or not isinstance(block_dura, (int, np.integer)) or not 1 <= block_dura <= FOLD_MAX:
        raise ValueError('%s: block_dura must be an int in [1, %d] (the rows one trial mean is made of), got %r'
                         % (who, FOLD_MAX, block_dura))
    if not isinstance(within, (bool, np.bool_)):
        raise ValueError('%s: within must be True or False, got %r' % (who, within))
    if not hasattr(label_runs, '__len__') or isinstance(label_runs, str) or len(label_runs) != R:
        raise ValueError('%s: label_runs must hold one sequence of condition names per run (%d runs)' % (who, R))
    groups = _runs.group_keys(groups, R, who)[0]
    if folds is None:
        folds = default_folds(groups, within)
    folds = np.asarray(folds)
    if folds.shape != (R,) or folds.dtype.kind not in 'iu':
        raise ValueError('%s: folds must hold one int per run (%d runs), got %s %r' % (who, R, folds.dtype, folds.shape))
    ev = events.match_events(label_runs, target_name, int(block_dura), TRstep=1, **match_kw)
    for r, T in enumerate(lengths):
        if len(label_runs[r]) != T:
            raise ValueError('%s: run %d has %d rows and %d condition names' % (who, r, T, len(label_runs[r])))
    if not ev.kept:
        raise ValueError('%s: no run yields a trial' % who)
    offs = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    idx = np.concatenate([i + offs[r] for r, i in zip(ev.kept, ev.index)])
    codes = np.concatenate(ev.labels)
    per = [len(l) for l in ev.labels]
    labels = np.asarray(ev.classes)[codes]
    tg = [groups[r] for r, n in zip(ev.kept, per) for _ in range(n)]
    tf = np.repeat(folds[ev.kept].astype(np.int64), per)
    return np.ascontiguousarray(idx, np.int64), labels, tg, tf, list(ev.classes)


def _event_patterns(planes, idx, M):
    """One float32 pattern per trial, ``[S, M]``: the mean of the trial's rows of the staged planes
    (chebgcn_gather_windows_indexed with one channel and ``fold`` = the rows of a trial; ``events.host_windows`` restates it)."""
    from . import ops
    return ops.gather_windows_indexed(planes, idx, M, 1, fold=int(idx.shape[1]))[:, 0, :M]


def _from_events(runs, label_runs, target_name, block_dura, groups, folds, within, kw, taken, refused, check, who):
    """What ``searchlight_events`` and ``crossnobis_events`` share: the runs as a list of ``[T, M]``; ``kw`` loses the ``match_events``
    keywords and ``device``, may name nothing outside ``taken``, and any of ``refused[0]`` is answered with ``refused[1]``; the trials
    of ``_events_plan`` (``folds`` as there, or a function of the number of runs); the caller's ``check(stand_in, labels, folds,
    groups, classes)`` on a stand-in of the patterns' shape, which do not exist yet; staging and the patterns' gather.  Returns
    ``(the checked arguments with the patterns, the device, whether every run came as a tensor)``."""
    malformed = 'runs must be a non-empty list of [T, M] arrays'
    runs, single, M, as_tensor = _runs.as_runs(runs, who, none=malformed, shape=malformed)
    if any(k in kw for k in refused[0]):
        raise ValueError(refused[1] % who)
    match_kw = {k: kw.pop(k) for k in _MATCH_KW if k in kw}
    unknown = set(kw) - set(taken) - {'device'}
    if unknown:
        raise ValueError('%s: unknown keyword %r' % (who, sorted(unknown)[0]))
    if single and label_runs is not None and len(label_runs) and isinstance(label_runs[0], str):
        label_runs = [label_runs]
    idx, labels, tg, tf, classes = _events_plan([int(r.shape[0]) for r in runs], label_runs, target_name, block_dura, groups,
                                                folds(len(runs)) if callable(folds) else folds, within, match_kw, who)
    device = kw.pop('device', None)
    a = check(np.zeros((idx.shape[0], M), np.float32), labels, tf, tg, classes)
    dev, planes = _runs.stage(runs, M, device, who)             # non-finite values: before the device is touched
    import torch
    with torch.cuda.device(dev):
        X = _event_patterns(planes, torch.as_tensor(idx).to(dev), M)
    return a._replace(X=X, tensor=True), dev, as_tensor


def searchlight_events(runs, label_runs, target_name, block_dura, neighbourhoods, groups=None, folds=None, within=True, **kw):
    """``searchlight`` on the trials of an event design: ``runs`` (one ``[T, M]`` array or a list; NumPy or torch) are staged
    as ``[Ttot, plane_stride(M)]`` planes (``runs.stage``, as for ``first_level``), ``match_events(label_runs, target_name, block_dura)``
    cuts the trials (its keywords ``start_trial``, ``hrf_delay``, ``flag_event``, ``rest`` pass through; ``TRstep`` does not:
    the pattern of a trial is the float32 mean of its ``block_dura <= 16`` rows, formed on the device by
    ``ops.gather_windows_indexed(..., C=1, fold=block_dura)`` -- ``events.host_windows(run, index, fold=block_dura)`` restates
    it bit for bit), and ``searchlight`` runs on the patterns with the classes of ``EventWindows.classes``.

    ``groups``: one key per run (the subject; default one group).  ``folds``: one int per run; default ``default_folds``: with
    ``within=True`` the run's position among its group's runs (leave-one-run-out), with ``within=False`` the group's index
    (leave-one-subject-out).  Every other keyword is ``searchlight``'s, ``classifier``, ``shrinkage`` and the SVM's ``C``,
    ``loss``, ``tol``, ``max_iter`` and ``return_solver`` included.  Returns NumPy maps, or device tensors if every run came as a
    tensor."""
    who = 'searchlight_events'
    mine = dict(scores=False, predictions=False, batch_centres=None, return_solver=False)
    mine.update((k, kw.pop(k)) for k in tuple(mine) if k in kw)                # kw keeps the classifier's and _from_events' keywords

    def check(stand_in, labels, tf, tg, classes):
        a = _check(stand_in, labels, neighbourhoods, tf, tg, within, classes, mine['scores'], mine['predictions'],
                   mine['batch_centres'], who, **kw)
        _solver_flag(mine['return_solver'], a, who)
        return a
    refused = '%s: TRstep and classes are not taken (one pattern per trial; the classes are sorted(set(target_name)))'
    a, dev, as_tensor = _from_events(runs, label_runs, target_name, block_dura, groups, folds, within, kw, {'classifier', *_CLF_KW},
                                     (('TRstep', 'classes'), refused), check, who)
    return _searchlight(a, dev, mine['scores'], mine['predictions'], mine['batch_centres'], as_tensor, who,
                        bool(mine['return_solver']))


# ---- RSA: crossnobis distances per ball -----------------------------------------------------------------------------------------

class RDMResult(collections.namedtuple('RDMResult', 'rdm shrinkage classes pairs groups folds')):
    """What ``crossnobis`` returns.  ``rdm`` float64 [G, npairs, U]: the cross-validated Mahalanobis distance of every pair of
    classes at every centre, per group, pairs numbered row-major over a < b (``scipy.spatial.distance.squareform``'s order),
    ``npairs = C (C - 1) / 2``; ``shrinkage`` float64 [G, U]: the shrinkage used, -1 where the ball is degenerate (its distances
    are 0); ``classes``; ``pairs`` int64 [npairs, 2]: the class indices (a, b) of every pair; ``groups`` the G keys in order of
    first appearance; ``folds`` int64 [G]: the partitions of every group."""
    __slots__ = ()

    def square(self, g=0):
        """The RDMs of group ``g`` as symmetric matrices with a zero diagonal: [U, C, C]."""
        C, r = len(self.classes), self.rdm[g]
        if is_tensor(r):
            import torch
            out = torch.zeros((r.shape[1], C, C), dtype=r.dtype, device=r.device)
            a, b = (torch.as_tensor(self.pairs[:, i]).to(r.device) for i in (0, 1))
            out[:, a, b] = r.t()
            out[:, b, a] = r.t()
            return out
        out = np.zeros((r.shape[1], C, C), r.dtype)
        out[:, self.pairs[:, 0], self.pairs[:, 1]] = r.T
        out[:, self.pairs[:, 1], self.pairs[:, 0]] = r.T
        return out

    def model_maps(self, models, method='pearson'):
        """``compare_rdms(self.rdm, models, method)``: [G, Q, U], the maps ``map_test`` takes."""
        return compare_rdms(self.rdm, models, method)


_RdmArgs = collections.namedtuple('_RdmArgs', 'X tensor S M y classes indptr indices U gidx keys shrink cell cell_ptr folds')


def _check_rdm(samples, labels, neighbourhoods, partitions, groups, classes, shrinkage, batch_centres, who, limits=True):
    """Everything ``crossnobis`` can check without the samples' values.  ``cell`` of the result: the cell (group, partition) of
    every sample, cells numbered group by group (order of first appearance) and partition ascending inside a group;
    ``cell_ptr`` int64 [G + 1]; ``shrink``: the float, or -1.0 for ``'auto'``."""
    _own_keyword('shrinkage', shrinkage, who)
    X, tensor, S, M, y, classes, part, keys, gidx, indptr, indices, U = _front(
        samples, labels, neighbourhoods, partitions, 'partitions', ' (the run a pattern comes from)', groups, classes, batch_centres,
        who, limits)
    length = np.diff(indptr)
    if length.max() > LDA_PMAX:
        row = int(np.argmax(length > LDA_PMAX))
        raise ValueError('%s: neighbourhood %d holds %d vertices; served: rows of up to %d (a covariance per ball)'
                         % (who, row, length[row], LDA_PMAX))
    pvals, pidx = np.unique(part, return_inverse=True)
    cnt = np.zeros((len(keys), pvals.size, len(classes)), np.int64)
    np.add.at(cnt, (gidx, pidx, y), 1)
    present = cnt.sum(axis=2) > 0                               # [G, partitions]: the cells
    folds = present.sum(axis=1)
    if folds.min() < 2:
        g = int(np.argmax(folds < 2))
        raise ValueError('%s: group %r has only one partition (%d); a cross-validated distance needs two independent estimates'
                         % (who, keys[g], int(pvals[np.argmax(present[g])])))
    bad = np.argwhere(present[:, :, None] & (cnt == 0))
    if bad.size:
        g, f, c = (int(v) for v in bad[0])
        raise ValueError('%s: group %r, partition %d holds no sample of class %r (unbalanced designs are not served)'
                         % (who, keys[g], int(pvals[f]), classes[c]))
    number_of = np.cumsum(present.ravel()).reshape(present.shape) - 1
    cell = number_of[gidx, pidx]
    cell_ptr = np.concatenate([[0], np.cumsum(folds)]).astype(np.int64)
    if limits and int(cell_ptr[-1]) > NMAX:
        raise ValueError('%s: %d (group, partition) cells; served: up to %d' % (who, int(cell_ptr[-1]), NMAX))
    return _RdmArgs(X, tensor, S, M, y, classes, indptr, indices, U, gidx, keys, -1.0 if isinstance(shrinkage, str) else float(shrinkage),
                    cell, cell_ptr, folds.astype(np.int64))


def _pairs(C):
    return np.array([(a, b) for a in range(C) for b in range(a + 1, C)], np.int64).reshape(-1, 2)


def crossnobis_host(samples, labels, neighbourhoods, partitions, groups=None, classes=None, shrinkage=0.1, batch_centres=None,
                    device=None, return_scale=False):
    """``crossnobis`` restated in float64 NumPy / SciPy (no device; ``device`` and ``batch_centres`` are accepted and ignored),
    the obvious way: per group and per centre the ball's columns are sliced out, the cell means and the residuals about them
    formed with NumPy, ``Sigma`` factorised with ``scipy.linalg.cho_factor`` and the cell patterns whitened with
    ``solve_triangular``; the distance is the EXPLICIT double sum
    ``sum_{k != l} (u_ka - u_kb) . (u_la - u_lb) / (F (F - 1) P)`` over ordered pairs of different cells.  The samples are
    rounded to float32 first, as staging does.  Returns an ``RDMResult`` of NumPy arrays; with ``return_scale`` a pair of it
    and ``scale`` float64 [G, npairs, U] ``= kappa (t_ab + q_ab) / (F (F - 1) P)``, ``kappa`` the 2-norm condition number of
    that (group, centre)'s ``Sigma`` (1 where degenerate): the magnitude a float64 evaluation may be off by."""
    import scipy.linalg
    who = 'crossnobis_host'
    a = _check_rdm(samples, labels, neighbourhoods, partitions, groups, classes, shrinkage, batch_centres, who, limits=False)
    X = host_array(a.X, who).astype(np.float64)
    C, U, G = len(a.classes), a.U, len(a.keys)
    pairs = _pairs(C)
    rdm = np.zeros((G, len(pairs), U))
    scale = np.zeros((G, len(pairs), U))
    gam = np.full((G, U), -1.0)
    for g in range(G):
        cells = np.arange(a.cell_ptr[g], a.cell_ptr[g + 1])
        F = cells.size
        lists = [[np.flatnonzero((a.cell == k) & (a.y == c)) for c in range(C)] for k in cells]
        order = np.concatenate([l for per in lists for l in per])              # cell ascending, class ascending, sample order
        nkc = np.array([[l.size for l in per] for per in lists], np.float64)
        n = nkc.sum()
        for u in range(U):
            cols = a.indices[a.indptr[u]:a.indptr[u + 1]]
            P = cols.size
            A = X[:, cols]
            mu = np.stack([np.stack([A[l].sum(axis=0) / l.size for l in per]) for per in lists])       # [F, C, P]
            m = (nkc[:, :, None] * mu).sum(axis=(0, 1)) / n
            d = mu - m
            R = np.concatenate([A[l] - mu[k, c] for k, per in enumerate(lists) for c, l in enumerate(per)])
            assert R.shape == (order.size, P)
            S_ = R.T @ R / n
            tr = np.trace(S_)
            if not tr > 0:
                scale[g, :, u] = 0.0
                continue
            nu = tr / P
            gg = lda_shrinkage_host(R) if a.shrink < 0 else a.shrink
            Sigma = (1.0 - gg) * S_ + gg * nu * np.eye(P)
            try:
                L = scipy.linalg.cho_factor(Sigma, lower=True)[0]
                w = scipy.linalg.solve_triangular(L, d.reshape(F * C, P).T, lower=True).T.reshape(F, C, P)
                ev = np.linalg.eigvalsh(Sigma)
                kappa = float(ev[-1] / ev[0])
            except np.linalg.LinAlgError:
                continue
            if not (np.isfinite(w).all() and np.isfinite(kappa) and kappa > 0):
                continue
            gam[g, u] = gg
            for i, (ca, cb) in enumerate(pairs):
                delta = w[:, ca] - w[:, cb]                     # [F, P]
                acc = 0.0
                for k in range(F):
                    for l in range(F):
                        if k != l:
                            acc += float(delta[k] @ delta[l])
                rdm[g, i, u] = acc / (F * (F - 1) * P)
                tot = delta.sum(axis=0)
                scale[g, i, u] = kappa * (float(tot @ tot) + float((delta * delta).sum())) / (F * (F - 1) * P)
    res = RDMResult(rdm, gam, list(a.classes), pairs, list(a.keys), a.folds.copy())
    return (res, scale) if return_scale else res


def compare_rdms(rdm, models, method='pearson'):
    """How well the RDM of every (group, centre) follows each model RDM: ``rdm`` float64 [G, npairs, U] (``RDMResult.rdm``; NumPy
    or torch), ``models`` [Q, npairs] in the same pair order (``scipy.spatial.distance.squareform(D, checks=False)`` of a C x C
    model) -> float64 [G, Q, U], of the kind ``rdm`` is.  ``method='pearson'``: the correlation over the pairs,
    ``sum (x - mean x)(m - mean m) / sqrt(sum (x - mean x)^2 sum (m - mean m)^2)``, 0 where the RDM or the model is constant
    (all entries equal; with two classes always).  ``'cosine'``: ``sum x m / sqrt(sum x^2 sum m^2)``, 0 where either is all
    zero -- crossnobis distances have a meaningful zero, so the cosine does not throw the overall separation away.  Plain float64
    torch / NumPy, no kernel.  Group inference: ``map_test(compare_rdms(res.rdm, models)[:, q], A)``.  Spearman and other
    rank-based comparisons are out of scope."""
    who = 'compare_rdms'
    if method not in ('pearson', 'cosine'):
        raise ValueError("%s: method must be 'pearson' or 'cosine', got %r" % (who, method))
    tensor = is_tensor(rdm)
    x = rdm if tensor else np.asarray(rdm, np.float64)
    if x.ndim != 3 or x.shape[1] < 1:
        raise ValueError('%s: rdm must be [G, npairs, U], got shape %r' % (who, tuple(x.shape)))
    mod = np.asarray(models.detach().cpu().numpy() if is_tensor(models) else models, np.float64)
    if mod.ndim != 2 or mod.shape[0] < 1 or mod.shape[1] != x.shape[1] or not np.isfinite(mod).all():
        raise ValueError('%s: models must be finite [Q >= 1, npairs = %d], got shape %r' % (who, x.shape[1], mod.shape))
    if tensor:
        import torch
        x = x.to(torch.float64)
        mod = torch.as_tensor(mod).to(x.device)
        xp, amax, amin, sqrt, where = torch, (lambda v, ax: v.amax(dim=ax)), (lambda v, ax: v.amin(dim=ax)), torch.sqrt, torch.where
        total, zeros = (lambda v, ax: v.sum(dim=ax)), torch.zeros_like
    else:
        xp, amax, amin, sqrt, where = np, (lambda v, ax: v.max(axis=ax)), (lambda v, ax: v.min(axis=ax)), np.sqrt, np.where
        total, zeros = (lambda v, ax: v.sum(axis=ax)), np.zeros_like
    npairs = x.shape[1]
    if method == 'pearson':
        dead_x = amax(x, 1) == amin(x, 1)                       # [G, U]
        dead_m = amax(mod, 1) == amin(mod, 1)                   # [Q]
        x = x - total(x, 1)[:, None, :] / npairs
        mod = mod - total(mod, 1)[:, None] / npairs
    else:
        dead_x = amax(abs(x), 1) == 0
        dead_m = amax(abs(mod), 1) == 0
    num = xp.einsum('gpu,qp->gqu', x, mod)
    den = sqrt(total(x * x, 1))[:, None, :] * sqrt(total(mod * mod, 1))[None, :, None]
    dead = dead_x[:, None, :] | dead_m[None, :, None] | ~(den > 0)
    return where(dead, zeros(num), num / where(dead, zeros(den) + 1.0, den))


_RdmPlan = collections.namedtuple('_RdmPlan', 'order cell_ptr class_ptr class_idx NM')


def _rdm_plan(a):
    """The tables of the kernels: the samples sorted by cell (stable, so every list keeps the caller's order), and per
    (cell, class) its samples as positions in the sorted order."""
    C, NM = len(a.classes), int(a.cell_ptr[-1])
    order = np.argsort(a.cell * C + a.y, kind='stable')         # cell ascending, class ascending, the caller's order inside
    key = (a.cell * C + a.y)[order]
    class_ptr = np.searchsorted(key, np.arange(NM * C + 1), side='left')
    i32 = lambda v: np.ascontiguousarray(v, np.int32)
    return _RdmPlan(order, i32(a.cell_ptr), i32(class_ptr), i32(np.arange(a.S)), NM)


def _run_rdm(a, plan, Xt, batch_centres):
    """The launches of ``crossnobis``: fit with one model per cell (``eps = 0``: only its means are used), then the centres bucket
    by bucket of row length and batch by batch.  Returns device tensors ``(rdm [G, npairs, U], shrinkage [G, U])``."""
    import torch
    from . import ops
    dev = Xt.device
    t = _upload(a, plan, dev, 'class_ptr class_idx cell_ptr')
    C, U, G = len(a.classes), a.U, len(a.keys)
    par, _ = ops.searchlight_fit(Xt, a.S, t.class_ptr, t.class_idx, C, torch.zeros(plan.NM, dtype=torch.float64, device=dev))
    rdm = torch.zeros((G, C * (C - 1) // 2, U), dtype=torch.float64, device=dev)
    gam = torch.full((G, U), -1.0, dtype=torch.float64, device=dev)
    for bucket, rows in _row_batches(a, ops.searchlight_rdm_geometry()['buckets'], batch_centres, dev):
        ops.searchlight_rdm(Xt, a.S, t.rowptr, t.colidx, rows, bucket, t.cell_ptr, t.class_ptr, t.class_idx, C, par, a.shrink, rdm,
                            gamma_out=gam)
    return rdm, gam


def _crossnobis(a, dev, batch_centres, as_tensor, who):
    import torch
    plan = _rdm_plan(a)
    with torch.cuda.device(dev):
        rdm, gam = _run_rdm(a, plan, _staged(a, plan.order, dev, who), batch_centres)
    if not as_tensor:
        rdm, gam = rdm.cpu().numpy(), gam.cpu().numpy()
    return RDMResult(rdm, gam, list(a.classes), _pairs(len(a.classes)), list(a.keys), a.folds.copy())


def crossnobis(samples, labels, neighbourhoods, partitions, groups=None, classes=None, shrinkage=0.1, batch_centres=None, device=None):
    """The representational dissimilarity matrix of every ball, on the device: the cross-validated Mahalanobis ("crossnobis",
    Walther et al. 2016) distance of every pair of classes at every (group, centre) -- an ``RDMResult``.  Where ``searchlight``
    says WHERE the conditions can be told apart, this says HOW a region tells them apart; ``compare_rdms`` turns the RDMs into
    maps of agreement with model RDMs, which ``map_test`` takes for group inference.

    ``samples`` [S, M], ``labels`` [S], ``neighbourhoods``, ``groups`` (the subject; ``None``: one group), ``classes``,
    ``batch_centres`` and ``device`` as ``searchlight`` takes them, rows of P <= ``LDA_PMAX`` = 128 vertices
    ``v_0 < ... < v_{P-1}``; ``partitions`` [S] ints: the run a pattern comes from.  A *cell* is a (group, partition); group g
    has ``F_g >= 2`` cells, and every cell must hold at least one sample of every class.

    The quantity, per (group g, row), everything in float64 and every order fixed; n the number of samples of g:

    1. Cell means: ``mu_{k,c,v}`` the mean of class c in cell k (chebgcn_searchlight_fit with one model per cell, a chain in
       sample order); ``m_v = (sum_{k,c} n_kc mu_kcv) / n`` (k, then c ascending); ``d_kcv = mu_kcv - m_v``.
    2. Noise covariance of the residuals about the CELL means, ``r_sv = x_sv - mu_{k(s), y(s), v}``:
       ``S_ij = (sum_s r_si r_sj) / n`` over the group's samples, cell ascending, class ascending, sample order;
       ``nu = tr S / P``; ``Sigma = (1 - g) S + g nu I``.  ``shrinkage``: ``g`` in ``[SHRINK_MIN, 1]`` = [1e-6, 1], or ``'auto'``:
       the Ledoit-Wolf coefficient of these residuals, exactly the rule of ``classifier='lda'`` (``lda_shrinkage_host(R)``).
    3. Whitening: ``Sigma = L L^T`` by Cholesky; ``u_kc = L^-1 d_kc`` (a forward solve).
    4. The distance of classes a < b:  ``T_c = sum_k u_kc`` (k ascending);
       ``q_ab = sum_k sum_v (u_kav - u_kbv)^2`` (k outer, v ascending, one fma chain); ``t_ab = sum_v (T_av - T_bv)^2``;
       ``rdm_ab = (t_ab - q_ab) / (F_g (F_g - 1) P)`` -- the mean over ordered pairs of different cells ``k != l`` of
       ``(u_ka - u_kb) . (u_la - u_lb) / P``, which multiplies pattern differences from DIFFERENT runs only and is therefore
       unbiased: zero on average where two classes do not differ (and negative about as often as positive there).
    5. Degenerate balls -- ``tr S`` not > 0 or a Cholesky pivot not positive and finite: every distance of that (group, centre)
       is 0 and its reported shrinkage is -1; nothing is NaN.

    Returns NumPy arrays, or device tensors if ``samples`` came as a tensor.  The result does not depend on ``batch_centres``,
    on the order of the rows or on what else the call holds, bit for bit.

    ``ValueError`` before any launch: malformed shapes and dtypes, non-finite samples, a label outside ``classes``, an empty
    neighbourhood, a cell that lacks a class (naming the group, the partition and the class), a group with only one partition,
    a row of more than 128 vertices, more than 32 classes or fewer than 2, a ``shrinkage`` outside ``[1e-6, 1]`` that is not
    ``'auto'``.

    Out of scope: Spearman and other rank-based comparisons, noise ceilings, balls above 128 vertices, unbalanced designs (a
    cell that lacks a class), label-permutation nulls."""
    who = 'crossnobis'
    a = _check_rdm(samples, labels, neighbourhoods, partitions, groups, classes, shrinkage, batch_centres, who)
    if not a.tensor:
        a = a._replace(X=host_array(a.X, who))                  # non-finite values: before the device is touched
    return _crossnobis(a, _runs.cuda_device(device, a.X), batch_centres, a.tensor, who)


def crossnobis_events(runs, label_runs, target_name, block_dura, neighbourhoods, groups=None, **kw):
    """``crossnobis`` on the trials of an event design, the twin of ``searchlight_events``: ``runs`` are staged as planes,
    ``match_events(label_runs, target_name, block_dura)`` cuts the trials (its keywords ``start_trial``, ``hrf_delay``,
    ``flag_event``, ``rest`` pass through), the pattern of a trial is the float32 mean of its ``block_dura <= 16`` rows, formed
    on the device, and ``crossnobis`` runs on the patterns with the classes of ``EventWindows.classes``.  The partition of a
    pattern is the run it was cut from (its position in ``runs``); ``groups``: one key per run (the subject; default one group).
    Every other keyword (``shrinkage``, ``batch_centres``, ``device``) is ``crossnobis``'s.  Returns NumPy arrays, or device
    tensors if every run came as a tensor."""
    who = 'crossnobis_events'
    shrinkage, batch_centres = kw.get('shrinkage', 0.1), kw.get('batch_centres', None)
    check = lambda stand_in, labels, tp, tg, classes: _check_rdm(stand_in, labels, neighbourhoods, tp, tg, classes, shrinkage,
                                                                 batch_centres, who)
    refused = ('%s: TRstep, classes and partitions are not taken (one pattern per trial; the classes are sorted(set(target_name)); the '
               'partition is the run)')
    a, dev, as_tensor = _from_events(runs, label_runs, target_name, block_dura, groups, np.arange, True, kw,
                                     {'shrinkage', 'batch_centres'}, (('TRstep', 'classes', 'partitions'), refused), check, who)
    return _crossnobis(a, dev, batch_centres, as_tensor, who)
