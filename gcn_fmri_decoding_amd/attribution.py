"""Attribution maps of a model: ``saliency`` (input gradients), ``occlusion`` (score drops under masked vertex groups),
``shapley`` (sampled Shapley values of vertex groups) and ``gradcam`` (class activation maps at a conv layer), each with its
per-class mean ``*_maps``.  ``Attribution`` carries the eight methods and is a base of ``models_gcn.base_model``; ``Pass`` is
what the model's layers see while one of them runs."""
import contextlib

import numpy as np
import torch

from . import _lib, ops


def shapley_permutations(G, P, antithetic, seed):
    """The permutations of a ``shapley`` call: int32 ``[P, G]``, row p the order in which permutation p reveals the G groups.
    Drawn one after the other by ``np.random.RandomState(seed).permutation(G)`` (NumPy's global stream is not touched); with
    ``antithetic`` only the even rows are drawn and row 2i + 1 is row 2i reversed."""
    rs = np.random.RandomState(seed)
    perms = np.empty((P, G), np.int32)
    for p in range(P):
        perms[p] = perms[p - 1, ::-1] if antithetic and p % 2 else rs.permutation(G)
    return perms


class Pass(object):
    """The state of one attribution call, ``model._pass`` while it runs (None outside one).  While it is set, the layers hand
    out their variables detached -- no weight gradient, bias gradient or optimizer work can follow -- and the head runs on
    ``ops.FCInputGrad``.  ``layer``: the index of the conv layer whose output the input gradient stops at (Grad-CAM), None for
    a pass that differentiates to the input or not at all; ``act``: that output, once a forward made it."""
    __slots__ = ('layer', 'act')

    def __init__(self, layer=None):
        self.layer, self.act = layer, None

    def grad_mode(self, i):
        """Autograd for conv layer ``i``: off up to the layer whose output the gradient stops at."""
        return torch.no_grad() if (self.layer is not None and i <= self.layer) else contextlib.nullcontext()

    def tap(self, i, x):
        """Conv layer ``i``'s output ``x`` (plane storage) as the next stage reads it: at ``layer``, made the tensor the input
        gradient stops at and kept in ``act``."""
        if i != self.layer:
            return x
        self.act = x.detach().requires_grad_(True)
        return self.act


class Attribution(object):
    """The attribution methods of ``base_model``.  They use the model's ``stage``, ``_gather_padded``, ``as_internal``,
    ``_inference_storage`` and ``_cam_level``, its sizes (``_M0``, ``channel``, ``M``, ``p``, ``batch_size``), its input order
    table ``_order_dev`` and ``training_mode``; the layers read ``_pass``."""

    @contextlib.contextmanager
    def _attribution_pass(self, layer=None):
        """Everything run inside is one attribution pass: dropout off, ``_pass`` set (the gradient stopping at conv layer
        ``layer``'s output when given).  Whatever the body does, ``training_mode`` is restored and ``_pass`` is None after."""
        was_training = self.training_mode
        self.training_mode, self._pass = False, Pass(layer)
        try:
            yield self._pass
        finally:
            self.training_mode, self._pass = was_training, None

    # ---------------------------------------------------------------- what the three share

    def _pass_args(self, who, data, target, labels, score, batch_size, baseline=None):
        """Checks the arguments the attribution methods share, before any device work; returns (S, targets int64 [S] or None
        for 'predicted', labels, batch size, baseline as a device tensor or None).  ``who`` names the caller in the messages.
        The device is checked last: a caller's own checks come before this one."""
        if score not in ops.SCORES:
            raise ValueError(who + ': score must be one of %s, got %r' % (sorted(ops.SCORES), score))
        bs = self.batch_size if batch_size is None else batch_size
        if isinstance(bs, bool) or not isinstance(bs, (int, np.integer)) or not 1 <= bs <= 65535:
            raise ValueError(who + ': batch_size must be an int in [1, 65535], got %r' % (batch_size,))
        shape = tuple(int(d) for d in data.shape)
        want = (int(self._M0), int(self.channel))
        if len(shape) != 3 or shape[1:] != want or shape[0] == 0:
            raise ValueError(who + ': data must be [S, %d, %d] with S > 0, got %s' % (want + (shape,)))
        S, n_classes = shape[0], int(self.M[-1])

        def classes(v, what):
            a = np.asarray(v)
            if a.shape != (S,) or not np.issubdtype(a.dtype, np.integer):
                raise ValueError(who + ': %s must be an int array of shape [%d], got %s %s' % (what, S, a.dtype, a.shape))
            a = a.astype(np.int64)
            if a.min() < 0 or a.max() >= n_classes:
                raise ValueError(who + ': %s must lie in [0, %d); got %d ... %d' % (what, n_classes, a.min(), a.max()))
            return a
        if labels is not None:
            labels = classes(labels, 'labels')
        if isinstance(target, str):
            if target == 'predicted':
                targets = None
            elif target == 'label':
                if labels is None:
                    raise ValueError(who + ": target='label' needs labels")
                targets = labels
            else:
                raise ValueError(who + ": target must be 'predicted', 'label', an int or an int array, got %r" % target)
        elif isinstance(target, (int, np.integer)) and not isinstance(target, bool):
            if not 0 <= int(target) < n_classes:
                raise ValueError(who + ': target %d is not a class in [0, %d)' % (int(target), n_classes))
            targets = np.full(S, int(target), np.int64)
        else:
            targets = classes(target, 'target')
        if baseline is not None:
            baseline = np.asarray(baseline, np.float32)
            if baseline.shape != want:
                raise ValueError(who + ': baseline must be [%d, %d], got %s' % (want + (baseline.shape,)))
        if self.device.type != 'cuda':
            raise RuntimeError(who + ': the model has no device to run on (%s)' % self.device)
        return S, targets, labels, int(bs), torch.as_tensor(baseline).to(self.device) if baseline is not None else None

    def _class_vector(self, S, targets):
        """The int64 device vector of the class each of ``S`` windows is attributed to: ``targets`` where given, else left for
        the seed kernel to fill with the windows' own argmax."""
        return (torch.empty(S, dtype=torch.int64, device=self.device) if targets is None
                else torch.as_tensor(targets).to(self.device))

    def _class_means(self, rows, cls, labels):
        """Per-window rows (float32 ``[S, G]`` on the device, classes ``cls`` there and ``labels`` on the host) -> the per-class
        means float64 ``[C, G]`` and the counts: summed on the device in float64, windows in order."""
        acc = torch.zeros((int(self.M[-1]), rows.shape[1]), dtype=torch.float64, device=self.device)
        ops.occlusion_class_sums(rows, cls, acc)
        return self._means_of_sums(acc, labels)

    @staticmethod
    def _means_of_sums(acc, labels):
        """Device class sums float64 ``[C, ...]`` -> (the means on the host, the int64 counts ``[C]``)."""
        counts = np.bincount(labels, minlength=acc.shape[0]).astype(np.int64)
        maps = acc.cpu().numpy()
        maps /= np.maximum(counts, 1).reshape((-1,) + (1,) * (maps.ndim - 1))  # in place, one pass (a class without windows stays 0)
        return maps, counts

    # ---------------------------------------------------------------- saliency maps

    def saliency(self, data, target='predicted', score='logit', method='gradient', steps=32, baseline=None, batch_size=None,
                 labels=None):
        """Attribution of each window's class score to its inputs.  ``data``: ``[S, M, channel]`` as for ``predict`` (NumPy,
        or a tensor from ``stage()``), in the caller's vertex order.  Returns ``(attr, target)``: float32 ``[S, M, channel]`` in
        the order of ``data`` (fake vertices included) and the int64 class ``[S]`` each window was attributed to.

        * ``target``: ``'predicted'`` (the window's own argmax, ``prediction()``'s tie rule), ``'label'`` (the int array
          ``labels=`` ``[S]``), an int, or an int array ``[S]``; classes lie in ``[0, M[-1])``.
        * ``score``: ``'logit'`` (z_c) or ``'logprob'`` (log softmax(z)_c).
        * ``method``: ``'gradient'`` (ds/dx), ``'grad_x_input'`` (x * ds/dx), ``'integrated'`` ((x - x0) * the mean of ds/dx at
          x0 + a_j (x - x0), a_j = (j + 1/2)/steps; ``baseline`` x0: None = zeros, or ``[M, channel]``; the class is decided at
          x and held along the path).
        * Dropout is off.  ``batch_size`` (default the model's): rows of one pass -- windows for the first two methods (the last
          batch zero-padded like ``predict``), ``max(1, batch_size // steps)`` windows of ``steps`` rows each for
          ``'integrated'``.

        One pass per batch: the forward with the ReLU masks, then the training step's input-gradient kernels -- no weight or bias
        gradient, no optimizer, nothing the model keeps is written."""
        attr, cls, _ = self._saliency_run(data, target, labels, score, method, steps, baseline, batch_size)
        return attr.cpu().numpy(), cls.cpu().numpy()

    def saliency_maps(self, data, labels, absolute=False, score='logit', method='gradient', steps=32, baseline=None,
                      batch_size=None):
        """Per-class mean attribution: window w (target = its label) adds ``saliency``'s map -- ``|map|`` with ``absolute`` --
        to the sum of class ``labels[w]``.  Returns ``(maps, counts)``: float64 ``[C, M, channel]`` (C = M[-1]; the mean, zero
        for a class without windows) and int64 ``[C]``.  The sums run on the device in float64, windows in order within a
        batch, batches in order; the per-window maps never leave the device."""
        acc, _, labels = self._saliency_run(data, 'label', labels, score, method, steps, baseline, batch_size, True, absolute)
        return self._means_of_sums(acc, labels)

    def _saliency_run(self, data, target, labels, score, method, steps, baseline, batch_size, sums=False, absolute=False):
        """The passes of ``saliency`` / ``saliency_maps``: per batch, the forward with masks on inputs that need a gradient
        and variables that do not, the seed (the windows' classes, under 'predicted' their argmax), the input gradient
        (autograd over the library's layers), the reduction into per-window rows or, with ``sums``, float64 class sums.
        Returns (those rows ``[S, M, channel]`` or sums ``[C, M, channel]``, the classes int64 ``[S]``, labels), on the device.
        Every argument is checked before any device work: method, steps and the channel limit of the saliency kernels here,
        the shared ones in ``_pass_args``."""
        integrated = method == 'integrated'
        if method not in ops.SALIENCY_METHODS:
            raise ValueError('saliency: method must be one of %s, got %r' % (sorted(ops.SALIENCY_METHODS), method))
        if integrated and (isinstance(steps, bool) or not isinstance(steps, (int, np.integer)) or not 1 <= steps <= 65535):
            raise ValueError('saliency: steps must be an int in [1, 65535], got %r' % (steps,))
        if not _lib.lib().chebgcn_saliency_supported(int(self.channel)):
            raise ValueError('saliency: %d channels are more than the saliency kernels serve (chebgcn_saliency_supported)'
                             % int(self.channel))
        S, targets, labels, bs, base = self._pass_args('saliency', data, target, labels, score, batch_size, baseline)
        data_dev = self.stage(data)
        _, M, C = data_dev.shape
        attr = None if sums else torch.empty((S, M, C), dtype=torch.float32, device=self.device)
        acc = torch.zeros((int(self.M[-1]), M, C), dtype=torch.float64, device=self.device) if sums else None
        cls, predicted = self._class_vector(S, targets), targets is None
        m = int(steps) if integrated else 1
        wpp = max(1, bs // m) if integrated else bs
        R = wpp * m
        order = self._order_dev
        windows = torch.arange(S, dtype=torch.int32, device=self.device)
        rows = torch.empty((wpp, M, C), dtype=torch.float32, device=self.device) if attr is None else None
        with self._attribution_pass():
            if integrated and predicted:
                # the class is decided at x itself and held fixed along the path
                with torch.no_grad():
                    for begin in range(0, S, bs):
                        end = min(begin + bs, S)
                        logits = self._inference_storage(self.as_internal(self._gather_padded(data_dev, windows[begin:end], bs)), 1)
                        ops.saliency_seed(logits, None, 1, end - begin, score, cls_out=cls[begin:end], want_grad=False)
                predicted = False
            for begin in range(0, S, wpp):
                end = min(begin + wpp, S)
                nw, idx = end - begin, windows[begin:end]
                if integrated:
                    x = ops.saliency_path(data_dev, order, idx, base, R, m, M)
                else:
                    x = self._gather_padded(data_dev, idx, R)
                x.requires_grad_(True)
                with torch.enable_grad():
                    logits = self._inference_storage(self.as_internal(x), 1)
                dz = ops.saliency_seed(logits, None if predicted else cls[begin:end], m, nw * m, score,
                                       cls_out=cls[begin:end] if predicted else None)
                dx, = torch.autograd.grad(logits, x, dz)
                ops.saliency_reduce(dx, data_dev, order, idx, base, m, method, absolute,
                                    attr[begin:end] if attr is not None else rows[:nw],
                                    cls[begin:end] if sums else None, acc)
        return (acc if sums else attr), cls, labels

    # ---------------------------------------------------------------- occlusion maps

    def occlusion(self, data, target='predicted', score='logit', groups=None, baseline=None, batch_size=None, labels=None):
        """How much each window's class score falls when a group of its vertices is set to a baseline ("virtual lesion").
        ``data``: ``[S, M, channel]`` as for ``predict`` (NumPy, or a tensor from ``stage()``), in the caller's vertex order.
        Returns ``(drop, target)``: float32 ``[S, G]`` with ``drop[w, g] = s_c(x_w) - s_c(x_w with group g's vertices set to
        the baseline)``, and the int64 class ``[S]`` each window was scored for.

        * ``groups``: an int array ``[M]`` in the caller's order with values in ``[-1, G)``; ``-1`` never occludes a vertex, and
          every id in ``[0, G)`` must occur.  ``None``: one group per vertex (``G = M``, fake vertices included).  In the
          coarsening's tree order (``coarsening.perm_data`` data) ``groups = np.arange(M) >> j`` occludes the clusters of
          level ``j``, ``2**j`` vertices each.
        * ``baseline``: ``None`` (zeros) or ``[M, channel]`` in the caller's order.
        * ``target``, ``labels``, ``score``: as for ``saliency``.  The class is decided on the unoccluded window and held for
          all of its rows.
        * Dropout is off.  ``batch_size`` (default the model's): forward rows of one pass.  Rows are (window, group) pairs,
          ``G + 1`` per window (the window itself first), window-major: a pass may hold part of a window or several windows,
          and the last one is zero-padded like ``predict``.  A call costs ``S * (G + 1)`` forward rows.

        Only the inference kernels run, plus three small ones (chebgcn_occlusion_rows / _score, chebgcn_saliency_seed); nothing
        the model keeps is written."""
        drop, cls, _ = self._occlusion_run(data, target, labels, score, groups, baseline, batch_size)
        return drop.cpu().numpy(), cls.cpu().numpy()

    def occlusion_maps(self, data, labels, score='logit', groups=None, baseline=None, batch_size=None):
        """Per-class mean occlusion drop: window w (target = its label) adds its ``occlusion`` row to the sum of class
        ``labels[w]``.  Returns ``(maps, counts)``: float64 ``[C, G]`` (C = M[-1]; the mean, zero for a class without windows)
        and int64 ``[C]``.  The sums run on the device in float64, windows in order; the per-window table never leaves the
        device."""
        return self._class_means(*self._occlusion_run(data, 'label', labels, score, groups, baseline, batch_size))

    def _group_args(self, who, groups, outside):
        """Checks ``groups`` of ``occlusion`` / ``shapley`` (``who`` names the caller in the messages, ``outside`` says what -1
        means to it); returns the group of each vertex in the caller's order as int64 ``[M]`` and G."""
        M = int(self._M0)
        if groups is None:
            g = np.arange(M, dtype=np.int64)
        else:
            a = np.asarray(groups)
            if a.dtype == np.bool_ or not np.issubdtype(a.dtype, np.integer) or a.shape != (M,):
                raise ValueError(who + ': groups must be an int array of shape [%d], got %s %s' % (M, a.dtype, a.shape))
            g = a.astype(np.int64)
            if g.min() < -1:
                raise ValueError(who + ': groups must lie in [-1, G) (-1: %s); got %d' % (outside, g.min()))
            if g.max() < 0:
                raise ValueError(who + ': groups holds no group (every entry is -1)')
            empty = np.flatnonzero(np.bincount(g[g >= 0], minlength=int(g.max()) + 1) == 0)
            if len(empty):
                raise ValueError(who + ': groups must use every id in [0, %d); %d of them occur nowhere (first %d)'
                                 % (int(g.max()) + 1, len(empty), empty[0]))
        return g, int(g.max()) + 1

    def _group_table(self, g):
        """The groups ``g`` of ``_group_args`` as the kernels take them: the group of each internal position, int32 ``[Mp]`` on
        the device, -1 on the pad."""
        M = int(self._M0)
        gid = np.full(ops.plane_stride(M), -1, np.int32)
        gid[:M] = g[self._order] if self._order is not None else g
        return torch.as_tensor(gid).to(self.device)

    def _occlusion_args(self, data, target, labels, score, groups, baseline, batch_size):
        """Checks every argument of ``occlusion`` / ``occlusion_maps`` before any device work: its own (groups, the channel
        limit of the occlusion kernels), then the shared ones (``_pass_args``); returns those of ``_pass_args``, then the group
        of each internal position as int32 ``[Mp]`` on the device (-1 on the pad) and G."""
        g, G = self._group_args('occlusion', groups, 'never occluded')
        if not _lib.lib().chebgcn_occlusion_supported(int(self.channel)):
            raise ValueError('occlusion: %d channels are more than the occlusion kernels serve (chebgcn_occlusion_supported)'
                             % int(self.channel))
        shared = self._pass_args('occlusion', data, target, labels, score, batch_size, baseline)
        return shared + (self._group_table(g), G)

    def _occlusion_run(self, data, target, labels, score, groups, baseline, batch_size):
        """The passes of ``occlusion`` / ``occlusion_maps``: per pass of ``bs`` rows, the rows in plane storage, the forward
        (no autograd, the variables detached, the head on the library's kernels), the class of the windows whose own row is
        in the pass (under 'predicted' its argmax, else as given), and the drops.  Returns (the drops float32 ``[S, G]``, the
        classes int64 ``[S]``, labels), on the device."""
        S, targets, labels, bs, base, gid, G = self._occlusion_args(data, target, labels, score, groups, baseline, batch_size)
        data_dev = self.stage(data)
        M = data_dev.shape[1]
        cls, predicted = self._class_vector(S, targets), targets is None
        G1 = G + 1
        total = S * G1
        order = self._order_dev
        drop = torch.empty((S, G), dtype=torch.float32, device=self.device)
        ref = torch.empty(S, dtype=torch.float32, device=self.device)
        with self._attribution_pass(), torch.no_grad():
            for r0 in range(0, total, bs):
                x = ops.occlusion_rows(data_dev, order, gid, base, r0, bs, G, M)
                logits = self._inference_storage(self.as_internal(x), 1)
                if predicted:
                    w = -(-r0 // G1)                    # the first window whose own row is in this pass
                    off = w * G1 - r0
                    if w < S and off < bs:
                        ops.saliency_seed(logits[off:], None, G1, min(bs - off, total - w * G1), score, cls_out=cls[w:],
                                          want_grad=False)
                ops.occlusion_score(logits, r0, G, cls, score, ref, drop)
        return drop, cls, labels

    # ---------------------------------------------------------------- Shapley maps

    def shapley(self, data, target='predicted', score='logit', groups=None, baseline=None, permutations=16, antithetic=True,
                seed=0, batch_size=None, labels=None):
        """How each window's class score is shared among groups of its vertices: sampled Shapley values.  ``data``:
        ``[S, M, channel]`` as for ``predict`` (NumPy, or a tensor from ``stage()``), in the caller's vertex order.  Returns
        ``(phi, target)``: float32 ``[S, G]`` and the int64 class ``[S]`` each window was scored for.

        A permutation of the G groups defines G + 1 rows: row j holds the window's own values on the vertices of the
        permutation's first j groups (and of group -1) and the baseline elsewhere -- row 0 is the baseline window, row G the
        window itself.  ``phi[w, g]`` is the mean over the permutations of ``s_c(row pos(g) + 1) - s_c(row pos(g))``, ``pos(g)``
        the position of g in the permutation.  Every window's row sums to ``s_c(x_w) - s_c(baseline window)``, whatever the
        permutations; where ``occlusion`` shows a drop near zero for each of several redundant groups, these share what
        they carry together.

        * ``groups``, ``baseline``, ``target``, ``labels``, ``score``: as for ``occlusion`` (a vertex of group -1 always keeps
          its own value).  At most 4096 groups: use parcels or networks, not vertices.
        * ``permutations``: P in [1, 4096], drawn by ``shapley_permutations(G, P, antithetic, seed)`` and shared by every
          window of the call; ``antithetic``: permutation 2i + 1 is the reverse of permutation 2i (an odd P leaves the last one
          unpaired); ``seed``: an int in [0, 2**32).  A call is bit-reproducible.
        * Dropout is off.  ``batch_size`` (default the model's): forward rows of one pass.  Rows are (window, permutation,
          prefix) triples in that order: a pass may hold part of a window or several windows, and the last one is zero-padded
          like ``predict``.  A call costs ``S * P * (G + 1)`` forward rows, and ``S`` more under ``'predicted'`` (the class is
          decided by one plain forward over the windows first).

        Only the inference kernels run, plus four small ones (chebgcn_shapley_rows / _score / _reduce, chebgcn_saliency_seed);
        nothing the model keeps is written."""
        phi, cls, _ = self._shapley_run(data, target, labels, score, groups, baseline, permutations, antithetic, seed, batch_size)
        return phi.cpu().numpy(), cls.cpu().numpy()

    def shapley_maps(self, data, labels, score='logit', groups=None, baseline=None, permutations=16, antithetic=True, seed=0,
                     batch_size=None):
        """Per-class mean Shapley values: window w (target = its label) adds its ``shapley`` row to the sum of class
        ``labels[w]``.  Returns ``(maps, counts)``: float64 ``[C, G]`` (C = M[-1]; the mean, zero for a class without windows)
        and int64 ``[C]``.  The sums run on the device in float64, windows in order; the per-window table never leaves the
        device."""
        return self._class_means(*self._shapley_run(data, 'label', labels, score, groups, baseline, permutations, antithetic,
                                                    seed, batch_size))

    def _shapley_args(self, data, target, labels, score, groups, baseline, permutations, antithetic, seed, batch_size):
        """Checks every argument of ``shapley`` / ``shapley_maps`` before any device work: its own (permutations, antithetic,
        seed), the groups (as ``occlusion`` checks them, then the limits of the Shapley kernels), then the shared ones
        (``_pass_args``); returns those of ``_pass_args``, then the group of each internal position as int32 ``[Mp]`` on the
        device (-1 on the pad), G and the rank table int32 ``[P, G]`` on the device (the inverse of the permutations)."""
        def whole(v, lo, hi):
            return isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_)) and lo <= v < hi
        if not whole(permutations, 1, 4097):
            raise ValueError('shapley: permutations must be an int in [1, 4096], got %r' % (permutations,))
        if not isinstance(antithetic, (bool, np.bool_)):
            raise ValueError('shapley: antithetic must be True or False, got %r' % (antithetic,))
        if not whole(seed, 0, 2 ** 32):
            raise ValueError('shapley: seed must be an int in [0, 2**32), got %r' % (seed,))
        g, G = self._group_args('shapley', groups, 'outside the game')
        P = int(permutations)
        if G > 4096:
            raise ValueError('shapley: groups holds %d groups, more than the 4096 it serves (use parcels, not vertices)' % G)
        if P * (G + 1) >= 2 ** 31:
            raise ValueError('shapley: permutations * (G + 1) = %d rows per window, the limit is 2**31 - 1' % (P * (G + 1)))
        if not _lib.lib().chebgcn_shapley_supported(int(self.channel)):
            raise ValueError('shapley: %d channels are more than the Shapley kernels serve (chebgcn_shapley_supported)'
                             % int(self.channel))
        shared = self._pass_args('shapley', data, target, labels, score, batch_size, baseline)
        perms = shapley_permutations(G, P, bool(antithetic), int(seed))
        rank = np.empty_like(perms)
        np.put_along_axis(rank, perms, np.arange(G, dtype=np.int32)[None, :], axis=1)
        return shared + (self._group_table(g), G, torch.as_tensor(rank).to(self.device))

    def _shapley_run(self, data, target, labels, score, groups, baseline, permutations, antithetic, seed, batch_size):
        """The passes of ``shapley`` / ``shapley_maps``.  Under 'predicted', first one plain forward over the windows for their
        classes.  Then, per pass of ``bs`` consecutive rows: the rows in plane storage, the forward (no autograd, the variables
        detached, the head on the library's kernels), the scores into the table ``[windows, P, G + 1]``; one reduction once the
        table is complete.  A table above ``ops.SHAPLEY_TABLE_BYTES`` is run over as many windows at a time as fit.  Nothing
        waits for the device.  Returns (phi float32 ``[S, G]``, the classes int64 ``[S]``, labels), on the device."""
        S, targets, labels, bs, base, gid, G, rank = self._shapley_args(data, target, labels, score, groups, baseline,
                                                                        permutations, antithetic, seed, batch_size)
        data_dev = self.stage(data)
        M = data_dev.shape[1]
        cls = self._class_vector(S, targets)
        P = rank.shape[0]
        per = P * (G + 1)
        order = self._order_dev
        phi = torch.empty((S, G), dtype=torch.float32, device=self.device)
        chunk = min(S, max(1, ops.SHAPLEY_TABLE_BYTES // (4 * per)))
        table = torch.empty((chunk, P, G + 1), dtype=torch.float32, device=self.device)
        with self._attribution_pass(), torch.no_grad():
            if targets is None:
                windows = torch.arange(S, dtype=torch.int32, device=self.device)
                for begin in range(0, S, bs):
                    end = min(begin + bs, S)
                    logits = self._inference_storage(self.as_internal(self._gather_padded(data_dev, windows[begin:end], bs)), 1)
                    ops.saliency_seed(logits, None, 1, end - begin, score, cls_out=cls[begin:end], want_grad=False)
            for w0 in range(0, S, chunk):
                w1 = min(w0 + chunk, S)
                for r0 in range(0, (w1 - w0) * per, bs):
                    x = ops.shapley_rows(data_dev[w0:w1], order, gid, rank, base, r0, bs, M)
                    logits = self._inference_storage(self.as_internal(x), 1)
                    ops.shapley_score(logits, r0, cls[w0:w1], score, table[:w1 - w0])
                ops.shapley_reduce(table[:w1 - w0], rank, phi[w0:w1])
        return phi, cls, labels

    # ---------------------------------------------------------------- Grad-CAM maps

    def gradcam(self, data, layer=None, target='predicted', score='logit', method='gradcam', relu=True, batch_size=None,
                labels=None):
        """Class activation maps of each window at a conv layer.  ``data``: ``[S, M, channel]`` as for ``predict`` (NumPy, or a
        tensor from ``stage()``), in the caller's vertex order.  Returns ``(cam, target)``: float32 ``[S, M]`` at the input
        resolution in the order of ``data`` (fake vertices included), and the int64 class ``[S]`` each window was scored for.

        * ``layer``: ``'conv1'`` ... ``'conv<n>'``; ``None`` is the top conv layer.  Its activation ``A`` ``[F, N]`` is the
          layer's output as the next stage reads it (after bias, ReLU and pooling; ``finetuning_cgcnn``'s top layer before its
          pooling, as its flat head reads it) over the ``N`` vertices of that resolution, and ``G = ds/dA``.
        * ``method``: ``'gradcam'`` (``cam_i = sum_f alpha_f A[f, i]``, ``alpha_f`` the mean of ``G[f]`` over the ``N``
          vertices) or ``'grad_x_activation'`` (``cam_i = sum_f G[f, i] A[f, i]``).  ``relu``: ``max(0, cam)``.  At the top
          layer of a ``cgcnn`` the head reads the feature mean, so ``G[f, i] = g_i / F`` is the same for every filter and
          ``'gradcam'`` is ``ReLU(mean(alpha) * sum_f A[f, i])``: the per-vertex product is the map that stays informative there.
        * Level vertex ``j`` (the coarsening's tree order) covers the input vertices ``[j P, (j + 1) P)``, ``P`` the product of
          the pools up to the layer; each of them carries its value.
        * ``target``, ``labels``, ``score``, ``batch_size``: as for ``saliency`` (``method='gradient'``).  Dropout is off.

        One pass per batch: the layers up to ``layer`` without autograd, the layers above it, the head and the seed as a saliency
        pass runs them (input-gradient kernels only), the gradient taken at the layer's output, then chebgcn_gradcam_weights /
        _map.  Nothing the model keeps is written."""
        cam, cls, _ = self._gradcam_run(data, target, labels, score, layer, method, relu, batch_size)
        return cam.cpu().numpy(), cls.cpu().numpy()

    def gradcam_maps(self, data, labels, layer=None, score='logit', method='gradcam', relu=True, batch_size=None):
        """Per-class mean Grad-CAM map: window w (target = its label) adds its ``gradcam`` row to the sum of class ``labels[w]``.
        Returns ``(maps, counts)``: float64 ``[C, M]`` (C = M[-1]; the mean, zero for a class without windows) and int64 ``[C]``.
        The sums run on the device in float64, windows in order; the per-window maps never leave the device."""
        return self._class_means(*self._gradcam_run(data, 'label', labels, score, layer, method, relu, batch_size))

    def _gradcam_run(self, data, target, labels, score, layer, method, relu, batch_size):
        """The passes of ``gradcam`` / ``gradcam_maps``: per batch of ``bs`` windows (the last one zero-padded), the forward
        that stops autograd at the layer's output (``Pass.tap`` keeps it), the seed (the windows' classes, under 'predicted'
        their argmax), the gradient at that output, the map rows.  Returns (the maps float32 ``[S, M]``, the classes int64
        ``[S]``, labels), on the device.  Every argument is checked before any device work: layer, method and relu here, the
        shared ones in ``_pass_args`` (the channel limit of the saliency kernels does not apply: none of them runs)."""
        nl = len(self.p)
        names = ['conv%d' % (i + 1) for i in range(nl)]
        if layer is None:
            li = nl - 1
        elif isinstance(layer, str) and layer in names:
            li = names.index(layer)
        else:
            raise ValueError("gradcam: layer must be None or one of 'conv1' ... 'conv%d', got %r" % (nl, layer))
        if not isinstance(method, str) or method not in ops.GRADCAM_METHODS:
            raise ValueError('gradcam: method must be one of %s, got %r' % (sorted(ops.GRADCAM_METHODS), method))
        if not isinstance(relu, (bool, np.bool_)):
            raise ValueError('gradcam: relu must be True or False, got %r' % (relu,))
        S, targets, labels, bs, _ = self._pass_args('gradcam', data, target, labels, score, batch_size)
        data_dev = self.stage(data)
        cls, predicted = self._class_vector(S, targets), targets is None
        N, P, order = self._cam_level(li)
        windows = torch.arange(S, dtype=torch.int32, device=self.device)
        cam = torch.empty((S, data_dev.shape[1]), dtype=torch.float32, device=self.device)
        with self._attribution_pass(li) as ps:
            for begin in range(0, S, bs):
                end = min(begin + bs, S)
                nw = end - begin
                x = self._gather_padded(data_dev, windows[begin:end], bs)
                with torch.enable_grad():
                    logits = self._inference_storage(self.as_internal(x), 1)
                A, ps.act = ps.act, None
                dz = ops.saliency_seed(logits, None if predicted else cls[begin:end], 1, nw, score,
                                       cls_out=cls[begin:end] if predicted else None)
                G, = torch.autograd.grad(logits, A, dz)
                ops.gradcam_map(A, G, method, order, nw, N, P, relu, cam[begin:end])
        return cam, cls, labels
