"""Voxelwise encoding models on the device: a ridge regression from a wide feature matrix (delayed stimulus features, up to 256
columns) to every vertex, the penalty chosen per vertex (or per subject) by leave-one-run-out cross-validation, and the map of the
held-out R^2 or correlation -- the "voxelwise modelling" workflow of naturalistic fMRI, for which there is no event design
(chebgcn_ridge_*, include/chebgcn.h).

The scan is read once.  Every fold's fit and every held-out score is a function of three statistics of each run r, with ``Xc_r`` the
run's features centred per column and ``y_r`` a vertex's series: ``c_r = Xc_r^T y_r`` and the sum and the sum of squares of ``y_r``
(one ``chebgcn_glm_project`` over the table ``[Xc_r | 1]``), and ``G_r = Xc_r^T Xc_r`` (host).  For a fold with training sums
``(G_tr, c_tr)`` and held-out sums ``(G_te, c_te, tss_te)`` the ridge weights are ``w = (G_tr + alpha I)^-1 c_tr`` and the held-out
residual sum of squares is ``rss = tss_te - 2 w.c_te + w.G_te w``: no ``[T, M]`` prediction is ever formed.  Centring per run is
the per-run intercept of the literature; no intercept is returned.

Per model (every fold of every subject, and one model on all the subject's runs for the refit) the host factors
``G_tr = V diag(lambda) V^T`` (``numpy.linalg.eigh``) and hands the kernels ``V``, ``H = sym(V^T G_te V)`` and the reciprocals
``d[a][j] = 1 / (max(lambda_j, 0) + alpha_a)`` (``model_tables``); the kernels run the chains of ``model_chains`` /
``score_chains`` / ``select_chains`` / ``weight_chains`` below, which are their NumPy restatement bit for bit: every multiply
and add rounded on its own, every chain from 0 over ascending index.  ``ridge_cv_host`` runs the same chains on statistics formed
by ``@``; its yardstick in the tests fits and predicts explicitly.

Host-only at import: NumPy and the constants of ``_lib``; torch is imported by the functions that need it.
"""
import collections
import numbers

import numpy as np

from . import _lib, runs as _runs

SCORES = _lib.RIDGE_SCORES                   # 'r2', 'r'
FMAX, AMAX, RUNS_MAX, PANEL = 256, 32, 64, 64   # chebgcn_ridge_query(2 .. 4); the columns of one chebgcn_glm_project call


class EncodingResult(collections.namedtuple('EncodingResult', 'score alpha_index alphas weights scores groups folds')):
    """What ``ridge_cv`` / ``ridge_cv_host`` return (S subjects, M vertices, F features, A penalties).

    ``score``        float32 [S, M]: the mean over the subject's folds of the held-out score at the selected penalty
    ``alpha_index``  int32 [S, M]: the selected penalty, an index into ``alphas``
    ``alphas``       float64 [A] NumPy, as given
    ``weights``      float32 [S, F, M] or None: the refit on ALL the subject's runs at the selected penalty
    ``scores``       float32 [S, A, M] or None: the mean held-out score at every penalty
    ``groups``       the subjects' keys in order of first appearance
    ``folds``        per subject the held-out sets as used: lists of positions among the subject's runs

    ``score``, ``alpha_index``, ``weights`` and ``scores`` are device tensors when every run came as a tensor, else NumPy."""
    __slots__ = ()

    def predict(self, features, group=None):
        """``Xc @ weights[g]`` for one ``[T, F]`` feature matrix, centred per column like a run of the fit, and the subject with
        key ``group`` (default: the first): float32 [T, M], the product formed in float64."""
        if self.weights is None:
            raise ValueError('predict: the result holds no weights (weights=False)')
        g = 0 if group is None else list(self.groups).index(group) if group in self.groups else -1
        if g < 0:
            raise ValueError('predict: unknown group %r' % (group,))
        X = np.asarray(features, np.float64)
        W = self.weights[g]
        if X.ndim != 2 or X.shape[1] != W.shape[0] or not np.isfinite(X).all():
            raise ValueError('predict: features must be a finite [T, F = %d] matrix, got %r' % (W.shape[0], X.shape))
        Xc = X - X.sum(axis=0) / max(X.shape[0], 1)
        if _runs.is_tensor(W):
            import torch
            return (torch.as_tensor(Xc).to(W.device) @ W.to(torch.float64)).to(torch.float32)
        return (Xc @ W.astype(np.float64)).astype(np.float32)


def delay_features(X, delays):
    """A copy of ``X`` [T, F] per delay ``d`` (ints >= 0), shifted down by ``d`` rows and zero-filled at the top, side by side in
    delay-major order: float64 [T, F * len(delays)] (the finite-impulse-response features of an encoding model)."""
    X = np.asarray(X, np.float64)
    if X.ndim != 2:
        raise ValueError('delay_features: X must be [T, F], got shape %r' % (X.shape,))
    delays = list(delays)
    if not delays or any(isinstance(d, (bool, np.bool_)) or not isinstance(d, (int, np.integer)) or d < 0 for d in delays):
        raise ValueError('delay_features: delays must be ints >= 0, at least one, got %r' % (delays,))
    T, F = X.shape
    out = np.zeros((T, F * len(delays)), np.float64)
    for i, d in enumerate(delays):
        if d < T:
            out[d:, i * F:(i + 1) * F] = X[:T - d]
    return out


# ---- arguments ------------------------------------------------------------------------------------------------------------------

_Plan = collections.namedtuple('_Plan', 'runs M tensors Xc F alphas keys members folds score shared')


def _plan(runs, features, alphas, groups, folds, score, alpha, who, limits=True):
    """Everything that can be checked without the series' values."""
    runs, _, M, tensors = _runs.as_runs(runs, who, min_rows=2, rows='a run needs at least two time points')
    R = len(runs)
    if _runs.is_tensor(features) or isinstance(features, np.ndarray):
        features = [features] if features.ndim == 2 else list(features)
    features = list(features)
    if len(features) != R:
        raise ValueError('%s: features must hold one [T, F] matrix per run (%d runs, %d matrices)' % (who, R, len(features)))
    Xc, F = [], None
    for r, (y, X) in enumerate(zip(runs, features)):
        X = X.detach().cpu().numpy() if _runs.is_tensor(X) else np.asarray(X)
        if X.ndim != 2 or X.dtype.kind not in 'fiu' or X.shape[1] < 1:
            raise ValueError('%s: the features of run %d must be a real [T, F] matrix' % (who, r))
        X = X.astype(np.float64)
        if not np.isfinite(X).all():
            raise ValueError('%s: the features of run %d hold non-finite values' % (who, r))
        if X.shape[0] != int(y.shape[0]):
            raise ValueError('%s: the features of run %d have %d rows, the run %d' % (who, r, X.shape[0], int(y.shape[0])))
        if F is None:
            F = int(X.shape[1])
        if X.shape[1] != F:
            raise ValueError('%s: run %d has %d features, run 0 has %d' % (who, r, X.shape[1], F))
        Xc.append(np.ascontiguousarray(X - X.sum(axis=0) / X.shape[0]))
    if limits and F > FMAX:
        raise ValueError('%s: F = %d features; served: F <= %d' % (who, F, FMAX))
    a = np.asarray(alphas)
    if a.ndim != 1 or a.size < 1 or a.dtype.kind not in 'fiu':
        raise ValueError('%s: alphas must be a vector of at least one number, got %r' % (who, alphas))
    a = a.astype(np.float64)
    if not (np.isfinite(a).all() and (a >= 0).all()):
        raise ValueError('%s: alphas must be finite and >= 0, got %r' % (who, alphas))
    if limits and a.size > AMAX:
        raise ValueError('%s: %d penalties; served: up to %d' % (who, a.size, AMAX))
    if score not in SCORES:
        raise ValueError("%s: score must be 'r2' or 'r', got %r" % (who, score))
    if alpha not in ('per_vertex', 'shared'):
        raise ValueError("%s: alpha must be 'per_vertex' or 'shared', got %r" % (who, alpha))
    _, keys, members = _runs.group_keys(groups, R, who)
    for g, mem in zip(keys, members):
        if len(mem) < 2:
            raise ValueError('%s: subject %r has %d run; cross-validation needs at least 2' % (who, g, len(mem)))
        if limits and len(mem) > RUNS_MAX:
            raise ValueError('%s: subject %r has %d runs; served: up to %d' % (who, g, len(mem), RUNS_MAX))
    if folds is None:
        folds = [[[i] for i in range(len(mem))] for mem in members]
    else:
        try:
            folds = [[[k for k in test] for test in sub] for sub in folds]
        except TypeError:
            raise ValueError('%s: folds must hold, per subject, a list of held-out sets of run positions' % who) from None
        if len(folds) != len(keys):
            raise ValueError('%s: folds must hold one list per subject (%d subjects, %d lists)' % (who, len(keys), len(folds)))
        for g, mem, sub in zip(keys, members, folds):
            if not sub:
                raise ValueError('%s: subject %r has no folds' % (who, g))
            for f, test in enumerate(sub):
                if any(isinstance(k, (bool, np.bool_)) or not isinstance(k, (int, np.integer)) or not 0 <= k < len(mem) for k in test):
                    raise ValueError('%s: fold %d of subject %r must hold run positions in [0, %d), got %r' % (who, f, g, len(mem), test))
                if not test or len(set(test)) != len(test):
                    raise ValueError('%s: fold %d of subject %r must hold at least one run, each once, got %r' % (who, f, g, test))
                if len(test) >= len(mem):
                    raise ValueError('%s: fold %d of subject %r holds out every run: the training set is empty' % (who, f, g))
        folds = [[sorted(int(k) for k in test) for test in sub] for sub in folds]
    if limits and sum(len(sub) + 1 for sub in folds) > 65535:
        raise ValueError('%s: %d models; served: up to 65535' % (who, sum(len(sub) + 1 for sub in folds)))
    return _Plan(runs, M, tensors, Xc, F, a, keys, members, folds, score, alpha == 'shared')


def _check_flags(weights, scores, batch_runs, who):
    for name, v in (('weights', weights), ('scores', scores)):
        if not isinstance(v, (bool, np.bool_)):
            raise ValueError('%s: %s must be True or False, got %r' % (who, name, v))
    if batch_runs is not None and (isinstance(batch_runs, (bool, np.bool_)) or not isinstance(batch_runs, (int, np.integer))
                                   or batch_runs < 1):
        raise ValueError('%s: batch_runs must be an int >= 1, got %r' % (who, batch_runs))


# ---- the tables of the models (host, float64: vertex-independent and tiny, like the GLM's SVD) -------------------------------------

def subject_models(n, folds):
    """The models of a subject of ``n`` runs: per fold ``(training positions, held-out positions)``, both ascending, then the
    model on all the runs, which holds nothing out."""
    return [(sorted(set(range(n)) - set(test)), list(test)) for test in folds] + [(list(range(n)), [])]


def model_tables(Xc, models, alphas):
    """The tables of the kernels for the models of one subject: ``Xc`` the centred features of its runs, ``models`` from
    ``subject_models`` -> ``(V [E, F, F], H [E, F, F], d [E, A, F])``, float64.

    ``G_tr`` / ``G_te`` are the sums of ``Xc_r^T Xc_r`` over the lists in order; ``lambda, V = eigh(G_tr)``;
    ``H = (V^T G_te V + its transpose) / 2``; ``d[a][j] = 1 / (max(lambda_j, 0) + alpha_a)``, and 0 where that denominator is at
    most ``F 2^-52 max(lambda)`` (the pseudo-inverse at alpha = 0).  A feature that is constant in every run of the subject (a
    zero row and column of every G) is left out of the factorisation and is its own eigenvector with lambda = 0, so that
    appending such a column changes no other number of any table, and through the chains no bit of any result."""
    F = int(Xc[0].shape[1])
    alphas = np.asarray(alphas, np.float64)
    keep = np.flatnonzero(sum((x * x).sum(axis=0) for x in Xc) > 0)
    Fk = int(keep.size)
    G = []
    for x in Xc:
        xk = np.ascontiguousarray(x[:, keep])
        G.append(xk.T @ xk)
    E, A = len(models), int(alphas.size)
    V = np.zeros((E, F, F))
    H = np.zeros((E, F, F))
    d = np.zeros((E, A, F))
    V[:] = np.eye(F)
    for e, (train, test) in enumerate(models):
        Gtr, Gte = np.zeros((Fk, Fk)), np.zeros((Fk, Fk))
        for r in train:
            Gtr = Gtr + G[r]
        for r in test:
            Gte = Gte + G[r]
        lam = np.zeros(F)
        if Fk:
            lk, Vk = np.linalg.eigh(Gtr)
            Hk = Vk.T @ Gte @ Vk
            V[e][np.ix_(keep, keep)] = Vk
            H[e][np.ix_(keep, keep)] = (Hk + Hk.T) / 2
            lam[keep] = lk
        den = np.maximum(lam, 0.0)[None, :] + alphas[:, None]
        floor = Fk * 2.0 ** -52 * max(float(lam.max()), 0.0)
        with np.errstate(divide='ignore'):
            d[e] = np.where(den > floor, 1.0 / np.where(den > floor, den, 1.0), 0.0)
    return V, H, d


# ---- the chains of the kernels, restated: plain float64 * and + in the stated order (include/chebgcn.h) -----------------------------

def tss_of(yy, s, T):
    """``tss = yy - s s / T`` of a run, 0 where it is below ``4 (T + 1) 2^-53 yy``: the round-off of that subtraction."""
    tss = yy - s * s / T
    return np.where(tss < 4.0 * (T + 1) * 2.0 ** -53 * yy, 0.0, tss)


def _list_sum(planes, runs):
    acc = np.zeros(planes.shape[1:], np.float64)
    for r in runs:
        if 0 <= r < planes.shape[0]:                            # (a run number out of range is skipped)
            acc = acc + planes[r]
    return acc


def _rotate(T, x):
    """``out_i = sum_j T[j][i] x_j``, one chain from 0 over ascending j per output; ``x`` [F, M]."""
    out = np.zeros_like(x)
    for j in range(T.shape[0]):
        out = out + T[j][:, None] * x[j][None, :]
    return out


def model_chains(c, train, test, V):
    """``chebgcn_ridge_rotate`` for one model: ``c`` float64 [R, F, M] -> ``(z, g)`` [F, M]."""
    return _rotate(V, _list_sum(c, train)), _rotate(V, _list_sum(c, test))


def score_chains(z, g, tss, H, d, score='r2'):
    """The score kernel of ``chebgcn_ridge_score`` for one fold model: ``tss`` [M] the held-out sum -> float64 [A, M]."""
    out = np.zeros((d.shape[0], z.shape[1]), np.float64)
    for a in range(d.shape[0]):
        w = d[a][:, None] * z
        h = _rotate(H, w)
        p = np.zeros(z.shape[1])
        q = np.zeros(z.shape[1])
        for i in range(z.shape[0]):
            p = p + w[i] * g[i]
            q = q + w[i] * h[i]
        with np.errstate(divide='ignore', invalid='ignore'):
            if score == 'r2':
                rss = (tss - 2.0 * p) + q
                out[a] = np.where(tss > 0, 1.0 - rss / np.where(tss > 0, tss, 1.0), 0.0)
            else:
                ok = (tss > 0) & (q > 0)
                out[a] = np.where(ok, p / np.sqrt(np.where(ok, tss * q, 1.0)), 0.0)
    return out


def select_chains(fold_values):
    """The selection of ``chebgcn_ridge_score`` for one subject: ``fold_values`` float64 [folds, A, M] ->
    ``(score float32 [M], alpha_index int32 [M], scores float32 [A, M])``."""
    n, A, M = fold_values.shape
    best = np.zeros(M)
    index = np.zeros(M, np.int32)
    scores = np.zeros((A, M), np.float32)
    for a in range(A):
        acc = np.zeros(M)
        for f in range(n):
            acc = acc + fold_values[f, a]
        mean = acc / n if n else acc
        scores[a] = mean.astype(np.float32)
        better = (mean > best) if a else np.ones(M, bool)
        best = np.where(better, mean, best)
        index = np.where(better, a, index).astype(np.int32)
    return best.astype(np.float32), index, scores


def weight_chains(z, Vt, d, index):
    """``chebgcn_ridge_weights`` for one subject: ``z`` of its all-runs model, ``Vt`` = V transposed, ``index`` int [M] (clamped
    into [0, A)) -> float32 [F, M]."""
    index = np.clip(np.asarray(index, np.int64), 0, d.shape[0] - 1)
    return _rotate(Vt, d[index].T * z).astype(np.float32)


def shared_index(scores):
    """``alpha='shared'``: the first penalty that maximises the float64 mean over vertices of the float32 table [A, M]."""
    return int(np.argmax(np.asarray(scores, np.float32).astype(np.float64).mean(axis=1)))


# ---- the two entry points ---------------------------------------------------------------------------------------------------------

def _lists(models):
    """The run lists of models as ``chebgcn_ridge_rotate`` takes them: ``(list_ptr int32 [2 E + 1], list_runs int32)``."""
    ptr, flat = [0], []
    for train, test in models:
        flat += list(train)
        ptr.append(len(flat))
        flat += list(test)
        ptr.append(len(flat))
    return np.asarray(ptr, np.int32), np.asarray(flat, np.int32)


def ridge_cv_host(runs, features, alphas, groups=None, folds=None, score='r2', alpha='per_vertex', weights=True, scores=False):
    """``ridge_cv`` on the host in NumPy float64: the statistics by ``@``, the tables of ``model_tables`` and the restated chains
    of the kernels.  No limits on F, the number of penalties or the runs of a subject.  Returns an ``EncodingResult`` of NumPy
    arrays."""
    who = 'ridge_cv_host'
    _check_flags(weights, scores, None, who)
    plan = _plan(runs, features, alphas, groups, folds, score, alpha, who, limits=False)
    host = [_runs.host_array(r, who, any_dtype=True).astype(np.float64) for r in plan.runs]
    S, M, F, A = len(plan.keys), plan.M, plan.F, plan.alphas.size
    out_score = np.zeros((S, M), np.float32)
    out_index = np.zeros((S, M), np.int32)
    out_scores = np.zeros((S, A, M), np.float32) if scores else None
    out_weights = np.zeros((S, F, M), np.float32) if weights else None
    for s, (mem, sub) in enumerate(zip(plan.members, plan.folds)):
        Xc = [plan.Xc[r] for r in mem]
        c = np.stack([x.T @ host[r] for x, r in zip(Xc, mem)])
        tss = np.stack([tss_of((host[r] * host[r]).sum(axis=0), host[r].sum(axis=0), float(host[r].shape[0])) for r in mem])
        models = subject_models(len(mem), sub)
        V, H, d = model_tables(Xc, models, plan.alphas)
        values = np.zeros((len(sub), A, M))
        for e, (train, test) in enumerate(models[:-1]):
            z, g = model_chains(c, train, test, V[e])
            values[e] = score_chains(z, g, _list_sum(tss, test), H[e], d[e], plan.score)
        sc, idx, table = select_chains(values)
        if plan.shared:
            best = shared_index(table)
            sc, idx = table[best].copy(), np.full(M, best, np.int32)
        out_score[s], out_index[s] = sc, idx
        if scores:
            out_scores[s] = table
        if weights:
            z, _ = model_chains(c, models[-1][0], [], V[-1])
            out_weights[s] = weight_chains(z, np.ascontiguousarray(V[-1].T), d[-1], idx)
    return EncodingResult(out_score, out_index, plan.alphas, out_weights, out_scores, list(plan.keys), plan.folds)


def ridge_cv(runs, features, alphas, groups=None, folds=None, score='r2', alpha='per_vertex', weights=True, scores=False,
             device=None, batch_runs=None):
    """Cross-validated ridge encoding models of every vertex, on the device.

    ``runs``       a list of ``[T_r, M]`` scans (NumPy arrays or torch tensors, any lengths >= 2, one M), as ``first_level`` takes them
    ``features``   one finite ``[T_r, F]`` matrix per run, one F <= 256; every column is centred per run on the host in float64, so
                   the model is fitted and scored on signals centred per run and has no intercept
    ``alphas``     1 to 32 finite penalties >= 0, in the order given (0 gives the pseudo-inverse)
    ``groups``     one key per run, the subject; every subject gets its own model and needs 2 to 64 runs
    ``folds``      None: leave one run out inside each subject; else per subject a list of held-out sets, each a list of positions
                   among that subject's runs, non-empty and leaving a non-empty training set
    ``score``      'r2' (``1 - rss / tss`` of the held-out runs) or 'r' (Pearson correlation of the centred held-out signal and
                   its prediction); a vertex that is constant in the held-out runs scores 0 there
    ``alpha``      'per_vertex': every vertex the first penalty that maximises its mean score over the folds; 'shared': one penalty
                   per subject, the first that maximises the float64 mean over vertices of the float32 table of mean scores
    ``weights``    also refit on all the subject's runs at the selected penalty: float32 [S, F, M]
    ``scores``     also return the mean score at every penalty: float32 [S, A, M]
    ``batch_runs`` runs per pass of the statistics kernel (default: what fits a quarter of the free device memory)

    One subject is resident at a time: its staged scans, its statistics (``8 (F + 1) Mp`` bytes a run) and the workspace of its
    models (``16 F Mp`` bytes a model).  The statistics are ``chebgcn_glm_project`` over ``[Xc_r | 1]`` in calls of at most 64
    columns; the total sum of squares ``tss_r = yy_r - s_r s_r / T_r`` with the project's floor.  Everything after is float64 with
    one order per sum (include/chebgcn.h), each output rounded once.  Results are bit-identical under any ``batch_runs``, under a
    permutation of the subjects, from call to call, between NumPy and tensor input, and when a feature that is constant in every
    run is appended.  Every argument error and every non-finite host array raises ``ValueError`` before any launch; nothing is
    NaN for finite input.  Returns an ``EncodingResult``."""
    who = 'ridge_cv'
    _check_flags(weights, scores, batch_runs, who)
    plan = _plan(runs, features, alphas, groups, folds, score, alpha, who)
    staged = [r if _runs.is_tensor(r) else _runs.host_array(r, who, any_dtype=True) for r in plan.runs]
    import torch
    from . import ops
    S, M, F, A = len(plan.keys), plan.M, plan.F, int(plan.alphas.size)
    Mp = _lib.plane_stride(M)
    dev = _runs.cuda_device(device, next((r for r in plan.runs if _runs.is_tensor(r) and r.is_cuda), None))
    limit = int(_lib.lib().chebgcn_glm_query(8))

    def put(a):
        return torch.as_tensor(np.ascontiguousarray(a)).to(dev)

    with torch.cuda.device(dev):
        out_score = torch.empty((S, M), dtype=torch.float32, device=dev)
        out_index = torch.empty((S, M), dtype=torch.int32, device=dev)
        out_scores = torch.empty((S, A, M), dtype=torch.float32, device=dev) if scores else None
        out_weights = torch.empty((S, F, M), dtype=torch.float32, device=dev) if weights else None
        for s, (mem, sub) in enumerate(zip(plan.members, plan.folds)):
            mine = [staged[r] for r in mem]
            _, planes = _runs.stage(mine, M, dev, who, any_dtype=True)
            offs = _runs.offsets(mine)
            n = len(mem)
            c = torch.empty((n, F, Mp), dtype=torch.float64, device=dev)
            ones = torch.empty((n, Mp), dtype=torch.float64, device=dev)
            yy = torch.empty((n, Mp), dtype=torch.float64, device=dev)
            batch = _runs.batch_size(batch_runs, n, limit, 8 * (min(F + 1, PANEL) + 1) * Mp, dev)
            for r0, r1, rows, o in _runs.batches(planes, offs, batch):
                table = np.concatenate([np.concatenate([plan.Xc[r], np.ones((plan.Xc[r].shape[0], 1))], axis=1)
                                        for r in mem[r0:r1]])
                for k0 in range(0, F + 1, PANEL):               # (a chain does not depend on the call's k: the cut is invisible)
                    k1 = min(k0 + PANEL, F + 1)
                    a, q2 = ops.glm_project(rows, o, M, put(table[:, k0:k1]))
                    kf = min(k1, F) - k0                        # feature columns of this call; the ones column is the last of all
                    if kf > 0:
                        c[r0:r1, k0:k0 + kf] = a[:, :kf]
                    if k1 == F + 1:
                        ones[r0:r1] = a[:, -1]
                    if k0 == 0:
                        yy[r0:r1] = q2
            T = put(np.diff(offs).astype(np.float64))[:, None]
            tss = yy - ones * ones / T                          # (three roundings: elementwise float64, as tss_of)
            tss = torch.where(tss < (4.0 * (T + 1.0) * 2.0 ** -53) * yy, torch.zeros_like(tss), tss)
            models = subject_models(n, sub)
            V, H, d = model_tables([plan.Xc[r] for r in mem], models, plan.alphas)
            ptr, flat = _lists(models)
            ptr, flat, dd = put(ptr), put(flat), put(d)
            ws, nbytes = ops.ridge_rotate(c, ptr, flat, put(V), M)
            fold_ptr = put(np.asarray([0, len(sub)], np.int32))
            sc, idx, table, _ = ops.ridge_score(ws, nbytes, tss, ptr, flat, put(H), dd, fold_ptr, M, len(sub), plan.score,
                                                scores=scores or plan.shared)
            if plan.shared:
                best = shared_index(table[0].cpu().numpy())     # (the host's own selection code, on the float32 table)
                sc, idx = table[:, best], torch.full((1, M), best, dtype=torch.int32, device=dev)
            out_score[s], out_index[s] = sc[0], idx[0]
            if scores:
                out_scores[s] = table[0]
            if weights:
                all_model = put(np.asarray([len(sub)], np.int32))
                out_weights[s] = ops.ridge_weights(ws, nbytes, put(V.transpose(0, 2, 1)), dd, all_model, idx.contiguous(), M)[0]
        if not plan.tensors:
            out_score, out_index = out_score.cpu().numpy(), out_index.cpu().numpy()
            out_scores = out_scores.cpu().numpy() if scores else None
            out_weights = out_weights.cpu().numpy() if weights else None
        return EncodingResult(out_score, out_index, plan.alphas, out_weights, out_scores, list(plan.keys), plan.folds)
