"""Grad-CAM maps (cgcnn.gradcam / gradcam_maps) on the host: the float64 restatement the GPU tests compare against, checked
here against central finite differences of the score in a layer's activation, the top-layer property of 'gradcam' on a cgcnn
and the upsampling rule; the argument checks of the public methods, which raise before any device work (on a shape-only
model); the library's declarations of the two kernels.  No GPU."""
import os
import re

import numpy as np
import pytest
import torch

from gcn_fmri_decoding_amd import _lib
from gcn_fmri_decoding_amd import graph as graph_mod
from gcn_fmri_decoding_amd import models_gcn
from test_saliency_host import SPECS, RefNet, _setup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class CamRefNet(RefNet):
    """RefNet with cgcnn.gradcam in float64.  ``head='mean'``: cgcnn's feature mean and FC head; ``head='flat'``:
    finetuning_cgcnn's, the top layer unpooled and flattened as [S, M*F] (element m*F + f) into newfc1 ... newlogits."""

    head = 'mean'
    tap = None          # (layer index, fn): fn(h) replaces that layer's output in the forward

    def logits(self, P, x):
        h = x
        nl = len(self.p)
        for i in range(nl):
            pre = self.conv(i, h, P['conv%d/weights' % (i + 1)]) + P['conv%d/bias' % (i + 1)]
            self._decision(pre.detach().numpy(), pre)
            h = torch.relu(pre)
            pp = self.p[i] if (self.head == 'mean' or i + 1 < nl) else 1
            if pp > 1:
                S, M, F = h.shape
                hr = h.reshape(S, M // pp, pp, F)
                if self.pool == 'mpool1':
                    v = hr.detach().numpy()
                    first = np.argmax(v, axis=2)[:, :, None, :]      # the first maximum
                    top2 = np.sort(v, axis=2)[:, :, -2:, :]
                    self._decision(np.where(top2[:, :, 1] > 0, top2[:, :, 1] - top2[:, :, 0], np.inf), pre)
                    h = hr.gather(2, torch.as_tensor(first)).squeeze(2)
                else:
                    h = hr.mean(dim=2)
            if self.tap is not None and self.tap[0] == i:
                h = self.tap[1](h)
        if self.head == 'mean':
            h, names = h.mean(dim=2), ['fc%d' % (i + 1) for i in range(len(self.M) - 1)] + ['logits']
        else:
            h, names = h.reshape(h.shape[0], -1), ['newfc%d' % (i + 1) for i in range(len(self.M) - 1)] + ['newlogits']
        for i, scope in enumerate(names):
            h = h @ P[scope + '/weights'] + P[scope + '/bias']
            if i + 1 < len(self.M):
                self._decision(h.detach().numpy(), h)
                h = torch.relu(h)
        return h

    def activation(self, P, x, layer, target, score):
        """(A, G) at layer index ``layer``: its output [S, N, F] and d score / d A, in float64."""
        got = {}

        def grab(h):
            h = h.detach().clone().requires_grad_(True)
            got['A'] = h
            return h
        self.tap = (layer, grab)
        try:
            s = self.score(P, torch.as_tensor(x), target, score)
        finally:
            self.tap = None
        G, = torch.autograd.grad(s.sum(), got['A'])
        return got['A'].detach().numpy(), G.numpy()

    def gradcam(self, P, x, layer, target='predicted', score='logit', method='gradcam', relu=True):
        """(cam [S, M], target [S], level map [S, N]) of cgcnn.gradcam in float64; ``layer``: the conv layer's index.  Leaves
        ``margin`` [S] of the forward the gradient was taken in, and ``scale`` [S]: the largest sum of the magnitudes of the terms
        a map value adds up, ``sum_f mean_i |G[f, i]| |A[f, i]|`` ('gradcam') or ``sum_f |G[f, i] A[f, i]|`` -- what fp32
        arithmetic is accurate to.  (The mean over the vertices in alpha may cancel: where it does, the map is far smaller than
        its terms.)"""
        x = np.asarray(x, np.float64)
        S = x.shape[0]
        with torch.no_grad():
            z = self.logits(P, torch.as_tensor(x)).numpy()
        if isinstance(target, str):
            target = np.argmax(z, axis=1)
        target = np.broadcast_to(np.asarray(target, np.int64), (S,)).copy()
        self.margin = None
        A, G = self.activation(P, x, layer, target, score)
        if method == 'gradcam':
            cam = (A * G.mean(axis=1, keepdims=True)).sum(axis=2)
            terms = (np.abs(A) * np.abs(G).mean(axis=1, keepdims=True)).sum(axis=2)
        else:
            cam = (A * G).sum(axis=2)
            terms = np.abs(A * G).sum(axis=2)
        self.scale = terms.max(axis=1)
        if relu:
            cam = np.maximum(cam, 0)
        return np.repeat(cam, x.shape[1] // A.shape[1], axis=1), target, cam


def _cam_setup(name, seed=0):
    net0, P, x = _setup(name, seed)
    net = CamRefNet.__new__(CamRefNet)
    net.__dict__.update(net0.__dict__)
    return net, P, x


@pytest.mark.parametrize('name', sorted(SPECS))
@pytest.mark.parametrize('score', ['logit', 'logprob'])
def test_reference_activation_gradient_matches_finite_differences(name, score):
    net, P, x = _cam_setup(name)
    target = np.array([0, 1, 3]) % SPECS[name]['M'][-1]
    rs = np.random.RandomState(7)
    eps = 1e-6
    for layer in range(len(SPECS[name]['p'])):
        A, G = net.activation(P, x, layer, target, score)
        worst = 0.0
        for _ in range(12):
            s, i, f = rs.randint(A.shape[0]), rs.randint(A.shape[1]), rs.randint(A.shape[2])
            sc = []
            for d in (eps, -eps):
                Ad = A.copy()
                Ad[s, i, f] += d
                net.tap = (layer, lambda h, Ad=Ad: torch.as_tensor(Ad))
                try:
                    with torch.no_grad():
                        sc.append(float(net.score(P, torch.as_tensor(x), target, score)[s]))
                finally:
                    net.tap = None
            worst = max(worst, abs((sc[0] - sc[1]) / (2 * eps) - G[s, i, f]))
        scale = np.abs(G).max()
        assert scale > 0, (name, layer)
        assert worst <= 1e-6 * scale + 1e-9, '%s / %s / layer %d: %.3e of %.3e' % (name, score, layer, worst, scale)


@pytest.mark.parametrize('name', ['cheb_pooled_max', 'cheb_pooled_avg', 'fourier'])
def test_reference_top_layer_gradcam_is_the_filter_sum(name):
    """At the top layer of a cgcnn the head reads the feature mean: G[f, i] = g_i / F for every f, every alpha_f is the same,
    and Grad-CAM is ReLU(mean(alpha) * sum_f A[f, i]) -- the filters carry no weighting of their own."""
    net, P, x = _cam_setup(name)
    top = len(SPECS[name]['p']) - 1
    for score in ('logit', 'logprob'):
        _, t, cam = net.gradcam(P, x, top, score=score)
        A, G = net.activation(P, x, top, t, score)
        assert np.abs(G - G.mean(axis=2, keepdims=True)).max() <= 1e-14 * np.abs(G).max()
        alpha = G.mean(axis=1)                                  # [S, F]
        assert np.abs(alpha - alpha[:, :1]).max() <= 1e-14 * np.abs(alpha).max()
        want = np.maximum(alpha.mean(axis=1)[:, None] * A.sum(axis=2), 0)
        assert np.abs(cam - want).max() <= 1e-12 * np.abs(want).max()
        # the per-vertex product keeps the gradient's variation over the vertices: g_i / F * sum_f A[f, i], not a multiple of
        # the filter sum
        _, _, gx = net.gradcam(P, x, top, t, score, 'grad_x_activation', relu=False)
        assert np.abs(gx - G[:, :, 0] * A.sum(axis=2)).max() <= 1e-12 * np.abs(gx).max()
        ratio = G[:, :, 0][A.sum(axis=2) > 1e-3 * A.sum(axis=2).max()]
        assert np.ptp(ratio) > 1e-3 * np.abs(ratio).max()


def test_reference_upsampling_rule():
    """A level-l vertex j covers input vertices [j P, (j + 1) P), P the product of the pools up to the layer."""
    net, P, x = _cam_setup('cheb_pooled_max')
    for layer, pool in ((0, 2), (1, 4)):
        cam, _, level = net.gradcam(P, x, layer, method='grad_x_activation', relu=False)
        assert level.shape == (x.shape[0], x.shape[1] // pool)
        v = np.arange(x.shape[1])
        assert np.array_equal(cam, level[:, v // pool])


def test_model_level_of_each_layer():
    """cgcnn._cam_level: the vertices of each layer's output, the input vertices each covers, the order (None on the reference
    numbering of a shape-only model)."""
    Ls = graph_mod.synthetic_graph(64, k=4, levels=2, seed=1)[0]
    net = models_gcn.cgcnn({'device': 'meta'}, Ls, [4, 4, 4], [3, 3, 3], [1, 2, 2], [8, 5], channel=2, batch_size=4,
                           verbose=False)
    M0 = Ls[0].shape[0]
    assert [net._cam_level(i) for i in range(3)] == [(M0, 1, None), (M0 // 2, 2, None), (M0 // 4, 4, None)]


def test_a_pass_that_raises_leaves_no_pass_state():
    """Whatever the body of an attribution pass does, ``training_mode`` comes back as it was and ``_pass`` is None again."""
    Ls = graph_mod.synthetic_graph(64, k=4, levels=2, seed=1)[0]
    net = models_gcn.cgcnn({'device': 'meta'}, Ls, [4, 4, 4], [3, 3, 3], [1, 2, 2], [8, 5], channel=2, batch_size=4,
                           verbose=False)
    assert net._pass is None and net.training_mode is False
    for was_training in (True, False):
        for layer in (None, 1):
            net.training_mode = was_training
            with pytest.raises(ZeroDivisionError):
                with net._attribution_pass(layer) as ps:
                    assert net._pass is ps and ps.layer == layer and ps.act is None
                    assert net.training_mode is False
                    1 / 0
            assert net._pass is None and net.training_mode is was_training
    # and a pass that ends normally
    net.training_mode = True
    with net._attribution_pass():
        assert net._pass is not None and net.training_mode is False
    assert net._pass is None and net.training_mode is True


def _meta_model(channel=3):
    Ls = graph_mod.synthetic_graph(60, k=4, levels=0, seed=1)[0]
    return models_gcn.cgcnn({'device': 'meta'}, Ls * 2, [4, 4], [3, 3], [1, 1], [8, 5], channel=channel, batch_size=4,
                            verbose=False)


BAD = [
    (dict(layer='conv3'), 'layer'),
    (dict(layer='conv0'), 'layer'),
    (dict(layer=1), 'layer'),
    (dict(layer='logits'), 'layer'),
    (dict(method='gradcam++'), 'method'),
    (dict(method='gradient'), 'method'),
    (dict(relu=1), 'relu'),
    (dict(relu='yes'), 'relu'),
    (dict(score='prob'), 'score'),
    (dict(target=5), 'target'),
    (dict(target=-1), 'target'),
    (dict(target='label'), 'labels'),
    (dict(target='best'), 'target'),
    (dict(target=np.arange(5)), 'target'),
    (dict(target='label', labels=np.arange(6) + 1), 'labels'),
    (dict(batch_size=0), 'batch_size'),
    (dict(batch_size=65536), 'batch_size'),
    (dict(batch_size=2.5), 'batch_size'),
]


@pytest.mark.parametrize('kw,word', BAD)
def test_gradcam_arguments_raise_before_device_work(kw, word):
    net = _meta_model()
    with pytest.raises(ValueError, match=word) as e:
        net.gradcam(np.zeros((6, 60, 3), np.float32), **kw)
    assert str(e.value).startswith('gradcam: ')


@pytest.mark.parametrize('kw,word', [(kw, w) for kw, w in BAD if 'target' not in kw and 'labels' not in kw])
def test_gradcam_maps_arguments_raise_before_device_work(kw, word):
    net = _meta_model()
    with pytest.raises(ValueError, match=word):
        net.gradcam_maps(np.zeros((6, 60, 3), np.float32), np.arange(6) % 5, **kw)


def test_gradcam_checks_data_and_labels():
    net = _meta_model()
    with pytest.raises(ValueError, match='data'):
        net.gradcam(np.zeros((6, 59, 3), np.float32))
    with pytest.raises(ValueError, match='data'):
        net.gradcam(np.zeros((0, 60, 3), np.float32))
    with pytest.raises(ValueError, match='data'):
        net.gradcam(np.zeros((60, 3), np.float32))
    with pytest.raises(ValueError, match='labels'):
        net.gradcam_maps(np.zeros((6, 60, 3), np.float32), np.array([0, 1, 2, 3, 4, 5]))
    with pytest.raises(ValueError, match='labels'):
        net.gradcam_maps(np.zeros((6, 60, 3), np.float32), np.array([0, 1]))
    with pytest.raises(ValueError, match='labels'):
        net.gradcam_maps(np.zeros((6, 60, 3), np.float32), np.zeros(6))


def test_valid_arguments_reach_the_device_check():
    """Arguments that pass every check go on to the device: a shape-only model has none to run on."""
    net = _meta_model()
    x = np.zeros((6, 60, 3), np.float32)
    with pytest.raises(RuntimeError, match='device'):
        net.gradcam(x)
    with pytest.raises(RuntimeError, match='device'):
        net.gradcam(x, layer='conv1', target=np.arange(6) % 5, score='logprob', method='grad_x_activation', relu=False,
                    batch_size=65535)
    with pytest.raises(RuntimeError, match='device'):
        net.gradcam(x, layer='conv2', target='label', labels=np.arange(6) % 5, relu=np.bool_(True))
    with pytest.raises(RuntimeError, match='device'):
        net.gradcam_maps(x, np.arange(6) % 5, layer='conv1', batch_size=1)


def test_no_channel_limit():
    """The saliency kernels' channel limit does not apply: gradcam runs none of them."""
    x = np.zeros((2, 60, 127), np.float32)
    with pytest.raises(ValueError, match='channels'):
        _meta_model(127).saliency(x)
    with pytest.raises(RuntimeError, match='device'):
        _meta_model(127).gradcam(x)
    with pytest.raises(RuntimeError, match='device'):
        _meta_model(127).gradcam_maps(x, np.zeros(2, np.int64))


def test_kernels_declared_and_bound():
    header = open(os.path.join(ROOT, 'include', 'chebgcn.h')).read()
    for name in ('chebgcn_gradcam_weights', 'chebgcn_gradcam_map'):
        assert re.search(r'\bint %s\(' % name, header), name
        assert name in _lib.SIGNATURES, name
        assert getattr(_lib.lib(), name) is not None
