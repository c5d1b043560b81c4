"""How far a decoded window can be trusted: ``predict_mc``, Monte-Carlo dropout (Gal & Ghahramani) from ONE pass of the trunk.
``Uncertainty`` carries the method and is a base of ``models_gcn.base_model``; ``MCHead`` is what the model's head reads while a
call runs; ``dropout_keep`` / ``mc_measures`` / ``mc_host`` restate the mask, the reduction and the whole sampled head in NumPy.

The reference trains its head with ``tf.nn.dropout`` behind every hidden FC layer (models_gcn.py:674-682) and nowhere else, so
the conv trunk and ``fc1`` -- the only wide FC layer -- are deterministic: they run once per window.  Only the small layers behind
the first dropout site run once per sample, on chebgcn_fc_fwd_dropout, which forms the mask in registers from a counter-based
generator: a pure function of ``(seed, sample, site, window, feature)``.  The result depends on nothing else -- not on the batch
size, not on what was called before, not on torch's generators."""
import numpy as np
import torch

from . import _lib, ops
from .series import aug_draw, check_seed

MC_SITES = _lib.MC_SITES         # CHEBGCN_MC_SITES: dropout sites a sample's refill numbers leave room for
MEASURES = ('probabilities', 'labels', 'entropy', 'expected_entropy', 'mutual_information', 'agreement', 'votes')
LAUNCH_OUTPUTS = 1 << 20         # S * B * O of one chebgcn_fc_fwd_dropout launch


# ---------------------------------------------------------------------------------------------------------------- host restatements

def dropout_threshold(keep):
    """``(T, inv_keep)`` of a keep probability in (0, 1]: a feature is kept iff its draw ``u < T``,
    ``T = min(int(keep * 2**32), 2**32 - 1)`` from the float64 ``keep``; a kept value is ``x * inv_keep`` with
    ``inv_keep = float32(1 / keep)``."""
    keep = float(keep)
    if not 0.0 < keep <= 1.0:
        raise ValueError('dropout: keep must lie in (0, 1], got %r' % (keep,))
    return min(int(keep * 2.0 ** 32), 2 ** 32 - 1), np.float32(1.0 / keep)


def dropout_keep(seed, sample, layer, windows, I, keep):
    """The Monte-Carlo dropout mask (include/chebgcn.h): bool ``[len(windows), I]``, True where feature ``d`` of window
    ``windows[w]`` is kept in sample ``sample`` at dropout site ``layer`` (site j follows ``fc{j+1}``).  ``windows``: window
    numbers, taken modulo 2**32."""
    if not 0 <= int(layer) < MC_SITES:
        raise ValueError('dropout_keep: the dropout site must lie in [0, %d), got %r' % (MC_SITES, layer))
    T, _ = dropout_threshold(keep)
    w = (np.asarray(windows, np.int64) & 0xFFFFFFFF).astype(np.uint64)
    refill = (int(sample) * MC_SITES + int(layer)) & 0xFFFFFFFF
    u = aug_draw(seed, refill, w[:, None], np.arange(int(I), dtype=np.uint64)[None, :])
    return u < np.uint64(T)


def _nan_top(a):
    """``a`` with every NaN replaced by a value above everything else (+inf, and +inf itself lowered to the largest finite number
    so that a NaN still beats it)."""
    a = np.asarray(a, np.float64)
    return np.where(np.isnan(a), np.inf, np.where(np.isposinf(a), np.finfo(np.float64).max, a))


def _first_max(a):
    """Index of the first maximum along the last axis, a NaN counting as the largest value (torch.argmax's rule)."""
    return np.argmax(_nan_top(a), axis=-1)


def entropy_nats(p):
    """``-sum p log p`` along the last axis, with ``0 log 0 = 0``."""
    p = np.asarray(p, np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        t = np.where(p == 0, 0.0, -p * np.log(p))
    return t.sum(axis=-1)


def mc_measures(logits):
    """The float64 restatement of chebgcn_mc_reduce: sampled logits ``[S, n, C]`` -> dict of ``probabilities [n, C]`` (the mean
    of the samples' softmaxes), ``labels [n]`` (its first maximum), ``entropy`` (of the mean), ``expected_entropy`` (the mean of
    the samples' entropies), ``mutual_information`` (their difference, at least 0), ``votes [n, C]`` (samples whose logits have
    their first maximum at the class, a NaN counting as largest) and ``agreement`` (the share of the votes ``labels`` got)."""
    z = np.asarray(logits, np.float64)
    S, n, C = z.shape
    with np.errstate(invalid='ignore'):
        e = np.exp(z - z.max(axis=2, keepdims=True))                          # (a NaN in a row makes the whole row NaN)
        p = e / e.sum(axis=2, keepdims=True)
        mean_p = p.sum(axis=0) / S
        h, he = entropy_nats(mean_p), entropy_nats(p).sum(axis=0) / S
        mi = np.maximum(h - he, 0.0)                                          # (np.maximum keeps a NaN)
    arg = _first_max(z)                                                       # [S, n]
    votes = (arg[:, :, None] == np.arange(C)[None, None, :]).sum(axis=0).astype(np.int32)
    labels = _first_max(mean_p).astype(np.int64)
    agreement = votes[np.arange(n), labels] / float(S)
    return dict(probabilities=mean_p, labels=labels, entropy=h, expected_entropy=he, mutual_information=mi, votes=votes,
                agreement=agreement)


def head_layers(variables):
    """The scopes of a head's FC layers in order, read off a dict of variables: ``['fc1', ..., 'logits']``."""
    n = 0
    while 'fc%d/weights' % (n + 1) in variables:
        n += 1
    return ['fc%d' % (i + 1) for i in range(n)] + ['logits']


def mc_host(features, variables, windows, samples, seed, keep):
    """The sampled head and its reduction in float64 NumPy, given the trunk's features ``[n, M_top]`` (the input of ``fc1``):
    what ``predict_mc`` computes for the windows numbered ``windows``.  ``variables``: name -> array (``fc{i}/weights|bias``,
    ``logits/weights|bias``).  Returns ``mc_measures`` of the sampled logits plus ``logits [samples, n, C]``."""
    P = {k: np.asarray(v, np.float64) for k, v in variables.items()}
    scopes = head_layers(P)
    if len(scopes) < 2:
        raise ValueError('mc_host: a head without a hidden FC layer has no dropout site')
    _, inv_keep = dropout_threshold(keep)
    h1 = np.maximum(np.asarray(features, np.float64) @ P['fc1/weights'] + P['fc1/bias'], 0.0)
    out = []
    for s in range(int(samples)):
        h = h1
        for site, scope in enumerate(scopes[1:]):
            m = dropout_keep(seed, s, site, windows, h.shape[1], keep)
            h = np.where(m, h * np.float64(inv_keep), 0.0) @ P[scope + '/weights'] + P[scope + '/bias']
            if scope != 'logits':
                h = np.maximum(h, 0.0)
        out.append(h)
    z = np.stack(out)
    res = mc_measures(z)
    res['logits'] = z
    return res


# ---------------------------------------------------------------------------------------------------------------- the result

class MCResult(dict):
    """What ``predict_mc`` returns: a dict whose entries also read as attributes -- ``probabilities`` float32 ``[n, C]``,
    ``labels`` int64 ``[n]``, ``entropy``, ``expected_entropy``, ``mutual_information``, ``agreement`` float32 ``[n]``, ``votes``
    int32 ``[n, C]``, and ``logits`` float32 ``[S, n, C]`` where the samples were asked for."""

    def __getattr__(self, name):
        try:
            return self[name]
        except KeyError:
            raise AttributeError(name)


class MCHead(object):
    """The state of one ``predict_mc`` run over ``n`` windows, ``model._mc`` while it runs (None otherwise): the head then
    samples (``cgcnn._head`` hands it the trunk's features) and writes the windows' measures into this object's device buffers.
    Before every batch the caller says with ``at`` which windows the batch's rows are."""

    def __init__(self, model, n, samples, seed, keep, first_window=0, return_samples=False):
        self.S, self.seed, self.n, self.first = int(samples), int(seed), int(n), int(first_window)
        self.threshold, self.inv_keep = dropout_threshold(keep)
        dev, C = model.device, int(model.M[-1])
        f = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
        i = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)
        self.out = dict(probabilities=f(n, C), labels=i(n), entropy=f(n), expected_entropy=f(n), mutual_information=f(n),
                        agreement=f(n), votes=i(n, C))
        self.logits = f(self.S, n, C) if return_samples else None
        self.where = self.win = None

    def at(self, positions):
        """The next batch's rows are the run's windows ``positions`` (int array): results go there, and their window numbers
        ``first_window + positions`` enter the masks."""
        pos = np.asarray(positions, np.int64)
        self.where = torch.as_tensor(pos).to(self.out['entropy'].device)
        self.win = torch.as_tensor(((pos + self.first) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)).to(self.where.device)

    def head(self, model, x):
        """``cgcnn._head`` under Monte-Carlo dropout: ``fc1`` once, every layer behind it once per sample, the reduction.
        Returns the mean probabilities of the batch ``[B, C]``."""
        B = x.shape[0]
        if self.where is None or self.where.numel() != B:
            raise RuntimeError('predict_mc: a batch of %d rows without its window numbers' % B)
        scopes = ['fc%d' % (i + 1) for i in range(len(model.M) - 1)] + ['logits']
        var = lambda scope, leaf: model._params['%s/%s' % (scope, leaf)].detach()
        h = ops.fc_forward_native(x, var('fc1', 'weights'), var('fc1', 'bias'), True, 'predict_mc')
        widest = max(int(m) for m in model.M[1:])
        chunk = max(1, min(self.S, LAUNCH_OUTPUTS // (B * widest)))
        z = torch.empty((self.S, B, int(model.M[-1])), dtype=torch.float32, device=x.device)
        for s0 in range(0, self.S, chunk):
            ns = min(chunk, self.S - s0)
            hs = h                                                      # site 0: one input for every sample
            for site, scope in enumerate(scopes[1:]):
                hs = ops.fc_forward_dropout(hs, var(scope, 'weights'), var(scope, 'bias'), scope != 'logits', self.win, ns, s0,
                                            site, self.seed, self.threshold, self.inv_keep)
            z[s0:s0 + ns] = hs
        red = ops.mc_reduce(z)
        for k, v in red.items():
            self.out[k].index_copy_(0, self.where, v)
        if self.logits is not None:
            self.logits.index_copy_(1, self.where, z)
        self.where = self.win = None
        return red['probabilities']

    def result(self):
        res = MCResult((k, v.cpu().numpy()) for k, v in self.out.items())
        res['labels'] = res['labels'].astype(np.int64)
        if self.logits is not None:
            res['logits'] = self.logits.cpu().numpy()
        return res


# ---------------------------------------------------------------------------------------------------------------- the method

class Uncertainty(object):
    """``predict_mc`` of ``base_model``.  Uses the model's ``stage``, ``_gather``, ``as_internal``, ``_inference_storage``, its
    sizes (``_M0``, ``channel``, ``M``, ``batch_size``), ``dropout`` and ``training_mode``; the head reads ``_mc``."""

    def _mc_refusal(self):
        """Raises where Monte-Carlo dropout has nothing to sample in this model (``finetuning_cgcnn`` overrides it)."""
        if len(self.M) < 2:
            raise ValueError('predict_mc: a model with M = %r has no hidden FC layer, hence no dropout site to sample'
                             % (list(self.M),))
        if len(self.M) - 1 > MC_SITES:
            raise ValueError('predict_mc: %d dropout sites are more than the %d a sample numbers' % (len(self.M) - 1, MC_SITES))

    def _mc_args(self, who, samples, seed, keep, batch_size):
        """Everything about a Monte-Carlo run that can be refused before device work (``who`` names the calling method).
        Returns (samples, seed, keep, batch size)."""
        if isinstance(samples, bool) or not isinstance(samples, (int, np.integer)) or not 1 <= samples <= ops.MC_SAMPLES_MAX:
            raise ValueError('%s: samples must be an int in [1, %d], got %r' % (who, ops.MC_SAMPLES_MAX, samples))
        seed = check_seed(seed, 'the seed', who)
        if keep is None:
            keep = self.dropout
            if isinstance(keep, bool) or not isinstance(keep, (int, float, np.integer, np.floating)) or not 0.0 < float(keep) < 1.0:
                raise ValueError('%s: the model was built with dropout = %r, which keeps everything or nothing: pass keep= '
                                 '(the probability of keeping a feature, strictly inside (0, 1))' % (who, keep))
        elif isinstance(keep, bool) or not isinstance(keep, (int, float, np.integer, np.floating)) or not 0.0 < float(keep) < 1.0:
            raise ValueError('%s: keep must be a number strictly inside (0, 1), got %r' % (who, keep))
        bs = self.batch_size if batch_size is None else batch_size
        if isinstance(bs, bool) or not isinstance(bs, (int, np.integer)) or not 1 <= bs <= 65535:
            raise ValueError('%s: batch_size must be an int in [1, 65535], got %r' % (who, batch_size))
        self._mc_refusal()
        C = int(self.M[-1])
        if C > ops.MC_CLASSES_MAX:
            raise ValueError('%s: %d classes are more than chebgcn_mc_reduce serves (%d)' % (who, C, ops.MC_CLASSES_MAX))
        widest = max(int(m) for m in self.M)
        if int(bs) * widest > LAUNCH_OUTPUTS:
            raise ValueError('%s: a batch of %d windows times %d outputs is more than one launch of the FC kernels takes (%d): '
                             'lower batch_size' % (who, bs, widest, LAUNCH_OUTPUTS))
        # fc1 runs on chebgcn_fc_fwd with no other path behind it: its size is checked here, not after the trunk has run
        inputs = int(self._spec('fc1/weights').shape[0])
        if not _lib.lib().chebgcn_fc_fwd_supported(int(bs), inputs, int(self.M[0])):
            raise ValueError('%s: fc1 (%d windows x %d inputs x %d outputs) is outside the range of chebgcn_fc_fwd'
                             % (who, bs, inputs, int(self.M[0])))
        return int(samples), seed, float(keep), int(bs)

    def _mc_dict(self, mc, batch_size):
        """``decode_series``' ``mc=`` argument -> (samples, seed, keep), checked like ``predict_mc``'s keywords."""
        if not isinstance(mc, dict) or set(mc) - {'samples', 'seed', 'keep'}:
            raise ValueError("decode_series: mc must be a dict with the keys 'samples', 'seed', 'keep' (all optional), got %r"
                             % (mc,))
        return self._mc_args('decode_series(mc=)', mc.get('samples', 32), mc.get('seed', 0), mc.get('keep'), batch_size)[:3]

    def predict_mc(self, data, samples=32, seed=0, keep=None, batch_size=None, return_samples=False):
        """Monte-Carlo dropout: what the model predicts for every window of ``data`` (``[n, M, channel]`` as for ``predict``)
        and how sure it is, from ``samples`` stochastic passes of the head with dropout left on.

        Returns an ``MCResult`` (a dict that also reads by attribute):

        * ``probabilities`` float32 ``[n, C]``: the mean over the samples of softmax(logits); ``labels`` int64 ``[n]``: its
          first maximum.
        * ``entropy`` ``[n]``: H(mean probabilities), the total uncertainty; ``expected_entropy``: the mean of the samples'
          H(softmax), the part the data leave open whatever the weights; ``mutual_information``: their difference, the part
          that comes from the model itself (high for windows unlike anything it was trained on).  Nats; ``0 log 0 = 0``.
        * ``votes`` int32 ``[n, C]``: how many samples decided for each class (``prediction()``'s tie rule); ``agreement``
          ``[n]``: the share of the samples that decided for ``labels``.
        * ``logits`` float32 ``[samples, n, C]`` with ``return_samples``.

        ``keep``: the probability of keeping a feature, strictly inside (0, 1); default the model's ``dropout``
        (``ValueError`` where that is 1).  The mask of sample s at the dropout site behind ``fc{j+1}`` is a pure function of
        ``(seed, s, j, window, feature)`` with ``window`` the index in ``data`` (``uncertainty.dropout_keep``): the same call
        gives the same bits again, whatever ran before, and ``batch_size`` (default the model's; the last batch runs at its
        own size) changes nothing but which kernels a launch lands on.  No torch random numbers are drawn.

        Evaluation mode, no gradient; nothing the model keeps is written.  The trunk and ``fc1`` run ONCE per window, the
        layers behind them once per sample (chebgcn_fc_fwd_dropout: the mask never exists in memory), the measures come from
        one reduction (chebgcn_mc_reduce).  No vendor GEMM.  ``finetuning_cgcnn`` (no dropout in its head) raises
        ``NotImplementedError``; a model without a hidden FC layer raises ``ValueError``."""
        S, seed, keep, bs = self._mc_args('predict_mc', samples, seed, keep, batch_size)
        shape = tuple(int(d) for d in data.shape)
        want = (int(self._M0), int(self.channel))
        if len(shape) != 3 or shape[1:] != want or shape[0] == 0:
            raise ValueError('predict_mc: data must be [n, %d, %d] with n > 0, got %s' % (want + (shape,)))
        if self.device.type != 'cuda':
            raise RuntimeError('predict_mc: the model has no device to run on (%s)' % self.device)
        n = shape[0]
        data_dev = self.stage(data)
        mc = MCHead(self, n, S, seed, keep, 0, return_samples)
        was_training = self.training_mode
        self.training_mode, self._mc = False, mc
        try:
            with torch.no_grad():
                for b0 in range(0, n, bs):
                    pos = np.arange(b0, min(b0 + bs, n))
                    mc.at(pos)
                    self._inference_storage(self._gather(data_dev, torch.as_tensor(pos.astype(np.int32)).to(self.device)), 1)
        finally:
            self.training_mode, self._mc = was_training, None
        return mc.result()
