"""Saliency maps (cgcnn.saliency / saliency_maps) on the host: the float64 restatement the GPU tests compare against, checked
here against central finite differences and the completeness of integrated gradients, and the argument checks of the public
methods, which raise before any device work (on a shape-only model).  No GPU."""
import numpy as np
import pytest
import torch

from gcn_fmri_decoding_amd import graph as graph_mod
from gcn_fmri_decoding_amd import models_gcn


class RefNet:
    """cgcnn (lib_new/models_gcn.py:658-682) in float64 torch, for autograd: chebyshev5 by the recurrence on the rescaled
    Laplacian, fourier / spline through graph.fourier and bspline_basis, b1relu / b2relu, mpool1 / apool1, the feature mean and
    the FC head.  The training backward's conventions: ReLU'(0) = 0, the max-pool gradient goes to the first maximum.
    ``L``: the Laplacians of every level, as cgcnn takes them; variables by their reference names and shapes."""

    def __init__(self, L, F, K, p, M, filter='chebyshev5', brelu='b1relu', pool='mpool1'):
        self.F, self.K, self.p, self.M, self.filter, self.pool = list(F), list(K), list(p), list(M), filter, pool
        self.ops = []
        j = 0
        for i, pp in enumerate(p):
            Li = L[j]
            if filter == 'chebyshev5':
                Lr = graph_mod.rescale_L(Li, lmax=2).astype(np.float64).toarray()
                self.ops.append(torch.as_tensor(Lr))
            else:
                lamb, U = graph_mod.fourier(Li)
                Bs = None
                if filter == 'spline':
                    Bs = torch.as_tensor(np.asarray(models_gcn.bspline_basis(K[i], lamb, degree=3), np.float64))
                self.ops.append((torch.as_tensor(np.asarray(U, np.float64)), Bs))
            j += int(np.log2(pp)) if pp > 1 else 0

    def conv(self, i, h, W):
        S, M, Fin = h.shape
        Fout = self.F[i]
        if self.filter == 'chebyshev5':
            Lr, K = self.ops[i], self.K[i]
            T = [h]
            if K > 1:
                T.append(torch.einsum('ij,sjf->sif', Lr, h))
            for _ in range(2, K):
                T.append(2 * torch.einsum('ij,sjf->sif', Lr, T[-1]) - T[-2])
            X = torch.stack(T, dim=3).reshape(S, M, Fin * K)          # column fin*K + k
            return X @ W
        U, Bs = self.ops[i]
        if Bs is not None:
            W = Bs @ W
        W = W.reshape(M, Fout, Fin)
        xh = torch.einsum('jm,sjf->smf', U, h)
        yh = torch.einsum('mof,smf->smo', W, xh)
        return torch.einsum('jm,smo->sjo', U, yh)

    margin = None

    def _decision(self, dist, pre):
        """Tracks, per window, the distance ``dist`` of the nearest ReLU / max-pool decision to its switching point, relative
        to the window's scale ``max |pre|`` at that layer (``margin``: the minimum over every call since it was last reset).
        Where it is within the rounding of the arithmetic under test, a float32 run may take the other branch -- and either
        gradient is right for its branch."""
        d = np.abs(np.asarray(dist, np.float64)).reshape(len(dist), -1).min(axis=1)
        m = d / np.maximum(np.abs(pre.detach().numpy()).reshape(len(dist), -1).max(axis=1), 1e-300)
        self.margin = m if self.margin is None else np.minimum(self.margin, m)

    def logits(self, P, x):
        h = x
        for i in range(len(self.p)):
            pre = self.conv(i, h, P['conv%d/weights' % (i + 1)]) + P['conv%d/bias' % (i + 1)]
            self._decision(pre.detach().numpy(), pre)
            h = torch.relu(pre)
            pp = self.p[i]
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
        h = h.mean(dim=2)
        for i in range(len(self.M)):
            scope = 'logits' if i + 1 == len(self.M) else 'fc%d' % (i + 1)
            h = h @ P[scope + '/weights'] + P[scope + '/bias']
            if i + 1 < len(self.M):
                self._decision(h.detach().numpy(), h)
                h = torch.relu(h)
        return h

    def score(self, P, x, target, score):
        z = self.logits(P, x)
        if score == 'logprob':
            z = torch.log_softmax(z, dim=1)
        return z[torch.arange(z.shape[0]), torch.as_tensor(target)]

    def grad(self, P, x, target, score):
        x = x.detach().clone().requires_grad_(True)
        g, = torch.autograd.grad(self.score(P, x, target, score).sum(), x)
        return g

    def saliency(self, P, x, target='predicted', score='logit', method='gradient', steps=32, baseline=None):
        """(attr, target) of cgcnn.saliency in float64; x: [S, M, channel].  Leaves ``margin`` [S] over every point the
        gradients were taken at."""
        x = torch.as_tensor(np.asarray(x, np.float64))
        S = x.shape[0]
        with torch.no_grad():
            z = self.logits(P, x).numpy()
        if isinstance(target, str):
            target = np.argmax(z, axis=1)
        target = np.broadcast_to(np.asarray(target, np.int64), (S,)).copy()
        self.margin = None
        if method != 'integrated':
            g = self.grad(P, x, target, score)
            return (g if method == 'gradient' else x * g).numpy(), target
        x0 = torch.zeros_like(x[0]) if baseline is None else torch.as_tensor(np.asarray(baseline, np.float64))
        total = torch.zeros_like(x)
        for j in range(steps):
            total += self.grad(P, x0 + (j + 0.5) / steps * (x - x0), target, score)
        return ((x - x0) * total / steps).numpy(), target


def random_params(net_spec, channel, M0, seed):
    """Reference-shaped float64 variables of a cgcnn of this architecture (drawn here, not by a model)."""
    rs = np.random.RandomState(seed)
    F, K, p, M, flt, brelu = (net_spec[k] for k in ('F', 'K', 'p', 'M', 'filter', 'brelu'))
    P, fin, m = {}, channel, M0
    for i in range(len(F)):
        if flt == 'chebyshev5':
            shape = (fin * K[i], F[i])
        elif flt == 'fourier':
            shape = (m, F[i], fin)
        else:
            shape = (K[i], F[i] * fin)
        P['conv%d/weights' % (i + 1)] = rs.randn(*shape) * 0.5 / np.sqrt(fin * max(K[i], 1))
        P['conv%d/bias' % (i + 1)] = 0.1 * rs.randn(1, m if brelu == 'b2relu' else 1, F[i])
        fin, m = F[i], m // p[i]
    for i, width in enumerate(M):
        scope = 'logits' if i + 1 == len(M) else 'fc%d' % (i + 1)
        P[scope + '/weights'] = rs.randn(m, width) / np.sqrt(m)
        P[scope + '/bias'] = 0.1 * rs.randn(width)
        m = width
    return {k: torch.as_tensor(v) for k, v in P.items()}


SPECS = {
    'cheb_pooled_max': dict(N=40, levels=2, F=[4, 5], K=[3, 2], p=[2, 2], M=[6, 4], filter='chebyshev5', brelu='b2relu',
                            pool='mpool1'),
    'cheb_pooled_avg': dict(N=40, levels=2, F=[4, 5], K=[3, 2], p=[2, 2], M=[6, 4], filter='chebyshev5', brelu='b1relu',
                            pool='apool1'),
    'fourier': dict(N=30, levels=0, F=[3, 4], K=[1, 1], p=[1, 1], M=[4], filter='fourier', brelu='b1relu', pool='mpool1'),
    'spline': dict(N=30, levels=0, F=[3, 4], K=[5, 4], p=[1, 1], M=[4], filter='spline', brelu='b2relu', pool='mpool1'),
}
CHANNEL = 3


def _setup(name, seed=0):
    s = SPECS[name]
    Ls = graph_mod.synthetic_graph(s['N'], k=4, levels=s['levels'], seed=seed)[0]
    L = Ls + [Ls[-1]] * max(0, len(s['p']) - len(Ls))
    net = RefNet(L, s['F'], s['K'], s['p'], s['M'], s['filter'], s['brelu'], s['pool'])
    P = random_params(s, CHANNEL, L[0].shape[0], seed + 1)
    x = np.random.RandomState(seed + 2).randn(3, L[0].shape[0], CHANNEL)
    return net, P, x


@pytest.mark.parametrize('name', sorted(SPECS))
@pytest.mark.parametrize('score', ['logit', 'logprob'])
def test_reference_gradient_matches_finite_differences(name, score):
    net, P, x = _setup(name)
    target = np.array([0, 1, 3]) % SPECS[name]['M'][-1]
    g = net.grad(P, torch.as_tensor(x), target, score).numpy()
    rs = np.random.RandomState(7)
    eps = 1e-6
    worst = 0.0
    for _ in range(12):
        s, v, c = rs.randint(x.shape[0]), rs.randint(x.shape[1]), rs.randint(x.shape[2])
        xp, xm = x.copy(), x.copy()
        xp[s, v, c] += eps
        xm[s, v, c] -= eps
        with torch.no_grad():
            fd = (net.score(P, torch.as_tensor(xp), target, score)[s] - net.score(P, torch.as_tensor(xm), target, score)[s]) / (2 * eps)
        worst = max(worst, abs(float(fd) - g[s, v, c]))
    scale = np.abs(g).max()
    assert scale > 0
    assert worst <= 1e-6 * scale + 1e-9, '%s / %s: %.3e of %.3e' % (name, score, worst, scale)


@pytest.mark.parametrize('name', sorted(SPECS))
def test_reference_integrated_gradients_completeness(name):
    """sum(attr) = s(x) - s(x0) in the limit; the midpoint rule's error shrinks as the steps grow."""
    net, P, x = _setup(name)
    base = 0.3 * np.random.RandomState(9).randn(x.shape[1], x.shape[2])
    target = np.array([1, 0, 2]) % SPECS[name]['M'][-1]
    with torch.no_grad():
        ds = (net.score(P, torch.as_tensor(x), target, 'logit')
              - net.score(P, torch.as_tensor(np.broadcast_to(base, x.shape).copy()), target, 'logit')).numpy()
    errs = []
    for m in (4, 16, 64):
        attr, _ = net.saliency(P, x, target, 'logit', 'integrated', m, base)
        errs.append(np.abs(attr.reshape(x.shape[0], -1).sum(axis=1) - ds).max())
    scale = np.abs(ds).max()
    assert errs[2] < errs[0], errs
    assert errs[2] <= 2e-2 * scale, (errs, scale)


def test_reference_predicted_target_is_the_first_maximum():
    net, P, x = _setup('fourier')
    with torch.no_grad():
        z = net.logits(P, torch.as_tensor(x)).numpy()
    _, t = net.saliency(P, x)
    assert np.array_equal(t, np.argmax(z, axis=1))


def _meta_model(**kw):
    Ls = graph_mod.synthetic_graph(60, k=4, levels=0, seed=1)[0]
    return models_gcn.cgcnn({'device': 'meta'}, Ls * 2, [4, 4], [3, 3], [1, 1], [8, 5], channel=3, batch_size=4,
                            verbose=False, **kw)


BAD = [
    (dict(method='smoothgrad'), 'method'),
    (dict(score='prob'), 'score'),
    (dict(target=5), 'target'),
    (dict(target=-1), 'target'),
    (dict(target=True), 'target'),
    (dict(target='label'), 'labels'),
    (dict(target='best'), 'target'),
    (dict(target=np.arange(5)), 'target'),
    (dict(target=np.zeros(6)), 'target'),
    (dict(target=np.array([0, 1, 2, 3, 4, 5])), 'target'),
    (dict(method='integrated', steps=0), 'steps'),
    (dict(method='integrated', steps=2.5), 'steps'),
    (dict(baseline=np.zeros((60, 2))), 'baseline'),
    (dict(batch_size=0), 'batch_size'),
]


@pytest.mark.parametrize('kw,word', BAD)
def test_saliency_arguments_raise_before_device_work(kw, word):
    net = _meta_model()
    with pytest.raises(ValueError, match=word):
        net.saliency(np.zeros((6, 60, 3), np.float32), **kw)


def test_saliency_checks_data_and_labels():
    net = _meta_model()
    with pytest.raises(ValueError, match='data'):
        net.saliency(np.zeros((6, 59, 3), np.float32))
    with pytest.raises(ValueError, match='data'):
        net.saliency(np.zeros((6, 60, 2), np.float32))
    with pytest.raises(ValueError, match='labels'):
        net.saliency_maps(np.zeros((6, 60, 3), np.float32), np.array([0, 1, 2, 3, 4, 5]))
    with pytest.raises(ValueError, match='labels'):
        net.saliency_maps(np.zeros((6, 60, 3), np.float32), np.array([0, 1]))
    with pytest.raises(ValueError, match='score'):
        net.saliency_maps(np.zeros((6, 60, 3), np.float32), np.zeros(6, np.int64), score='x')


def test_valid_arguments_reach_the_device_check():
    """Arguments that pass every check go on to the device: a shape-only model has none to run on."""
    net = _meta_model()
    with pytest.raises(RuntimeError, match='device'):
        net.saliency(np.zeros((6, 60, 3), np.float32), target=np.arange(6) % 5, method='integrated', steps=4,
                     baseline=np.ones((60, 3)))
    with pytest.raises(RuntimeError, match='device'):
        net.saliency_maps(np.zeros((6, 60, 3), np.float32), np.arange(6) % 5, absolute=True)
    with pytest.raises(RuntimeError, match='device'):
        net.saliency(np.zeros((6, 60, 3), np.float32), target='label', labels=np.arange(6) % 5)


def test_channel_limit_is_checked_with_the_arguments():
    from gcn_fmri_decoding_amd import _lib
    assert _lib.lib().chebgcn_saliency_supported(126) == 1
    assert _lib.lib().chebgcn_saliency_supported(127) == 0
    assert _lib.lib().chebgcn_saliency_supported(0) == 0
    Ls = graph_mod.synthetic_graph(60, k=4, levels=0, seed=1)[0]
    net = models_gcn.cgcnn({'device': 'meta'}, Ls, [4], [3], [1], [5], channel=127, batch_size=4, verbose=False)
    with pytest.raises(ValueError, match='channels'):
        net.saliency(np.zeros((2, 60, 127), np.float32))
