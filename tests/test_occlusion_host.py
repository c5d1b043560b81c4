"""Occlusion maps (base_model.occlusion / occlusion_maps) on the host: the float64 restatement the GPU tests compare against,
checked here against a brute-force loop over explicitly masked windows, and the argument checks of the public methods, which
raise before any device work (on a shape-only model).  No GPU."""
import numpy as np
import pytest
import torch

from gcn_fmri_decoding_amd import _lib
from gcn_fmri_decoding_amd import graph as graph_mod
from gcn_fmri_decoding_amd import models_gcn
from test_saliency_host import SPECS, RefNet, _setup


class OccRefNet(RefNet):
    """RefNet with cgcnn.occlusion in float64."""

    def occlusion(self, P, x, groups=None, baseline=None, target='predicted', score='logit'):
        """(drop [S, G], target [S]) of cgcnn.occlusion: per window one forward of G + 1 rows, the window itself first, then
        each group set to the baseline.  Leaves ``margin`` [S] (RefNet's decision margin, the minimum over a window's rows) and
        ``scale`` [S] (max |z| of the window's own logits)."""
        x = np.asarray(x, np.float64)
        S, M, C = x.shape
        g = np.arange(M) if groups is None else np.asarray(groups, np.int64)
        G = int(g.max()) + 1
        x0 = np.zeros((M, C)) if baseline is None else np.asarray(baseline, np.float64)
        with torch.no_grad():
            z = self.logits(P, torch.as_tensor(x)).numpy()
        if isinstance(target, str):
            target = np.argmax(z, axis=1)
        target = np.broadcast_to(np.asarray(target, np.int64), (S,)).copy()
        drop, margin = np.empty((S, G)), np.empty(S)
        for w in range(S):
            rows = np.repeat(x[w][None], G + 1, axis=0)
            for k in range(G):
                sel = g == k
                rows[k + 1, sel] = x0[sel]
            self.margin = None
            with torch.no_grad():
                s = self.score(P, torch.as_tensor(rows), np.full(G + 1, target[w]), score).numpy()
            drop[w] = s[0] - s[1:]
            margin[w] = self.margin.min()
        self.margin, self.scale = margin, np.abs(z).max(axis=1)
        return drop, target


def _brute_force(net, P, x, groups, baseline, target, score):
    """One window, one group at a time: the masked window and the window itself, each scored alone."""
    S, M, C = x.shape
    G = int(groups.max()) + 1
    x0 = np.zeros((M, C)) if baseline is None else baseline
    out = np.empty((S, G))
    for w in range(S):
        with torch.no_grad():
            s0 = float(net.score(P, torch.as_tensor(x[w][None]), target[w:w + 1], score)[0])
            for k in range(G):
                xm = x[w].copy()
                xm[groups == k] = x0[groups == k]
                out[w, k] = s0 - float(net.score(P, torch.as_tensor(xm[None]), target[w:w + 1], score)[0])
    return out


@pytest.mark.parametrize('name', sorted(SPECS))
@pytest.mark.parametrize('score', ['logit', 'logprob'])
def test_reference_occlusion_matches_brute_force(name, score):
    net0, P, x = _setup(name)
    net = OccRefNet.__new__(OccRefNet)
    net.__dict__.update(net0.__dict__)
    M = x.shape[1]
    rs = np.random.RandomState(3)
    groups = rs.randint(-1, 6, M)
    groups[:6] = np.arange(6)                   # every id occurs; some vertices are never occluded
    base = 0.4 * rs.randn(M, x.shape[2])
    for grp, b in ((None, None), (groups, base), (np.arange(M) >> 2, None)):
        drop, t = net.occlusion(P, x, grp, b, 'predicted', score)
        want = _brute_force(net, P, x, np.arange(M) if grp is None else grp, b, t, score)
        assert drop.shape == want.shape
        assert np.abs(drop - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), (name, score)
    assert net.margin.shape == (3,) and net.scale.shape == (3,)


def test_reference_occlusion_is_zero_where_the_group_already_equals_the_baseline():
    net0, P, x = _setup('cheb_pooled_max')
    net = OccRefNet.__new__(OccRefNet)
    net.__dict__.update(net0.__dict__)
    M = x.shape[1]
    groups = np.arange(M) % 7
    x = x.copy()
    x[1, groups == 3] = 0.0                     # window 1: group 3 is already at the zero baseline
    base = np.random.RandomState(5).randn(M, x.shape[2])
    base[groups == 5] = x[2, groups == 5]       # window 2: group 5 already equals this baseline
    drop, _ = net.occlusion(P, x, groups, None, 'predicted', 'logprob')
    assert drop[1, 3] == 0.0
    assert np.abs(drop).max() > 0
    drop, _ = net.occlusion(P, x, groups, base, np.array([0, 1, 2]), 'logit')
    assert drop[2, 5] == 0.0
    assert np.count_nonzero(drop) >= drop.size - 1


def test_reference_targets_follow_saliency():
    net0, P, x = _setup('fourier')
    net = OccRefNet.__new__(OccRefNet)
    net.__dict__.update(net0.__dict__)
    _, t = net.occlusion(P, x)
    _, want = net.saliency(P, x)
    assert np.array_equal(t, want)
    _, t = net.occlusion(P, x, target=np.array([3, 0, 1]))
    assert np.array_equal(t, [3, 0, 1])


def _meta_model(channel=3):
    Ls = graph_mod.synthetic_graph(60, k=4, levels=0, seed=1)[0]
    return models_gcn.cgcnn({'device': 'meta'}, Ls * 2, [4, 4], [3, 3], [1, 1], [8, 5], channel=channel, batch_size=4,
                            verbose=False)


_holes = np.arange(60) % 4
_holes[_holes == 2] = 3                         # id 2 occurs nowhere
BAD = [
    (dict(score='prob'), 'score'),
    (dict(target=5), 'target'),
    (dict(target=-1), 'target'),
    (dict(target='label'), 'labels'),
    (dict(target='best'), 'target'),
    (dict(target=np.arange(5)), 'target'),
    (dict(target='label', labels=np.arange(6) + 1), 'labels'),
    (dict(groups=np.arange(59)), 'groups'),
    (dict(groups=np.arange(60).reshape(6, 10)), 'groups'),
    (dict(groups=np.arange(60, dtype=np.float32)), 'groups'),
    (dict(groups=np.ones(60, bool)), 'groups'),
    (dict(groups=np.arange(60) - 2), 'groups'),
    (dict(groups=-np.ones(60, np.int64)), 'groups'),
    (dict(groups=_holes), 'groups'),
    (dict(groups=[0] * 59 + [2]), 'groups'),
    (dict(baseline=np.zeros((60, 2))), 'baseline'),
    (dict(baseline=np.zeros(60 * 3)), 'baseline'),
    (dict(batch_size=0), 'batch_size'),
    (dict(batch_size=65536), 'batch_size'),
    (dict(batch_size=2.5), 'batch_size'),
    (dict(batch_size=True), 'batch_size'),
]


@pytest.mark.parametrize('kw,word', BAD)
def test_occlusion_arguments_raise_before_device_work(kw, word):
    net = _meta_model()
    with pytest.raises(ValueError, match=word) as e:
        net.occlusion(np.zeros((6, 60, 3), np.float32), **kw)
    assert str(e.value).startswith('occlusion: ')


@pytest.mark.parametrize('kw,word', [(kw, w) for kw, w in BAD if 'target' not in kw and 'labels' not in kw])
def test_occlusion_maps_arguments_raise_before_device_work(kw, word):
    net = _meta_model()
    with pytest.raises(ValueError, match=word):
        net.occlusion_maps(np.zeros((6, 60, 3), np.float32), np.arange(6) % 5, **kw)


def test_occlusion_checks_data_and_labels():
    net = _meta_model()
    with pytest.raises(ValueError, match='data'):
        net.occlusion(np.zeros((6, 59, 3), np.float32))
    with pytest.raises(ValueError, match='data'):
        net.occlusion(np.zeros((0, 60, 3), np.float32))
    with pytest.raises(ValueError, match='labels'):
        net.occlusion_maps(np.zeros((6, 60, 3), np.float32), np.array([0, 1, 2, 3, 4, 5]))
    with pytest.raises(ValueError, match='labels'):
        net.occlusion_maps(np.zeros((6, 60, 3), np.float32), np.array([0, 1]))
    with pytest.raises(ValueError, match='labels'):
        net.occlusion_maps(np.zeros((6, 60, 3), np.float32), np.zeros(6))


def test_valid_arguments_reach_the_device_check():
    """Arguments that pass every check go on to the device: a shape-only model has none to run on."""
    net = _meta_model()
    x = np.zeros((6, 60, 3), np.float32)
    with pytest.raises(RuntimeError, match='device'):
        net.occlusion(x)
    with pytest.raises(RuntimeError, match='device'):
        net.occlusion(x, target=np.arange(6) % 5, score='logprob', groups=np.arange(60) >> 3, baseline=np.ones((60, 3)),
                      batch_size=65535)
    with pytest.raises(RuntimeError, match='device'):
        net.occlusion(x, target='label', labels=np.arange(6) % 5, groups=np.where(np.arange(60) < 10, -1, np.arange(60) % 4))
    with pytest.raises(RuntimeError, match='device'):
        net.occlusion(x, target=2, groups=np.zeros(60, np.int32), batch_size=1)
    with pytest.raises(RuntimeError, match='device'):
        net.occlusion_maps(x, np.arange(6) % 5, groups=list(np.arange(60) % 6))


def test_channel_limit_is_checked_with_the_arguments():
    L = _lib.lib()
    assert L.chebgcn_occlusion_supported(125) == 1
    assert L.chebgcn_occlusion_supported(126) == 0
    assert L.chebgcn_occlusion_supported(1) == 1
    assert L.chebgcn_occlusion_supported(0) == 0
    assert L.chebgcn_occlusion_supported(-1) == 0
    with pytest.raises(ValueError, match='channels'):
        _meta_model(126).occlusion(np.zeros((2, 60, 126), np.float32))
    with pytest.raises(ValueError, match='channels'):
        _meta_model(126).occlusion_maps(np.zeros((2, 60, 126), np.float32), np.zeros(2, np.int64))
    with pytest.raises(RuntimeError, match='device'):
        _meta_model(125).occlusion(np.zeros((2, 60, 125), np.float32))
