"""Occlusion maps (base_model.occlusion / occlusion_maps, model_perf.occlusion_maps) on the MI355X against the float64
restatement of tests/test_occlusion_host.py, on the networks of tests/test_gpu_saliency.py -- the atlas shape at channel 3
and 15, a relabelled graph of more than 1024 vertices, pooled networks (through index maps too), fourier, spline and split
bf16 -- and on finetuning_cgcnn with a frozen and with a tuned trunk.  Also: the per-class maps, the kernels a call names,
what it must not launch, bit-identical reruns, batch-size invariance, the model's state and checkpoints.

The score is a forward quantity: a ReLU or max-pool decision within fp32 reach of its switching point moves it by no more
than that reach (both are continuous), so no window is exempt from the bound on that account; the margins are recorded.  A
window whose two largest float64 logits lie within fp32 reach of each other may be attributed to the other class under
'predicted': the restatement is scored for the class the GPU chose, and only the class comparison exempts such a window."""

import numpy as np
import pytest
import torch

from conftest import record_measured
from gcn_fmri_decoding_amd import _lib, models_gcn, ops
from test_gpu_saliency import BS, NETS, REL, S, WIDE_REL, _data, _laplacians, _model
from test_occlusion_host import OccRefNet

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
TIE = 1e-5                  # the two largest logits closer than this (of the window's scale): the class may differ in fp32


def _reference(name, net, cls=OccRefNet):
    s = NETS[name]
    ref = cls(_laplacians(name), s['F'], s['K'], s['p'], s['M'], s.get('filter', 'chebyshev5'), s.get('brelu', 'b1relu'),
              s.get('pool', 'mpool1'))
    P = {n: torch.as_tensor(net.variable(n).detach().cpu().numpy().astype(np.float64)) for n in net.variables()}
    return ref, P


def _group_sets(M):
    rs = np.random.RandomState(6)
    holes = rs.randint(-1, 5, M)
    holes[:5] = np.arange(5)                    # ids 0..4 all occur; about a sixth of the vertices never occluded
    sets = {'cluster': np.arange(M) >> (3 if M <= 400 else 5), 'holes': holes}
    if M <= 128:
        sets['vertex'] = None
    return sets


def _check(tag, net, ref, P, x, drop, t, target, score, groups, baseline, bound, labels=None):
    """drop / t of one call against the float64 restatement, scored for the GPU's classes; returns the per-window errors."""
    want, _ = ref.occlusion(P, x, groups, baseline, t, score)
    assert drop.dtype == np.float32 and drop.shape == want.shape and t.dtype == np.int64 and t.shape == (len(x),)
    with torch.no_grad():
        z = ref.logits(P, torch.as_tensor(x.astype(np.float64))).numpy()
    zs = np.sort(z, axis=1)
    gap = (zs[:, -1] - zs[:, -2]) / ref.scale
    if isinstance(target, str) and target == 'predicted':
        clear = gap > TIE
        assert np.array_equal(t[clear], np.argmax(z, axis=1)[clear]), (tag, t, np.argmax(z, axis=1), gap)
    elif isinstance(target, str):
        assert np.array_equal(t, labels)
    else:
        assert np.array_equal(t, np.broadcast_to(target, t.shape))
    err = np.abs(drop.astype(np.float64) - want).max(axis=1) / ref.scale
    record_measured('occlusion_vs_float64', case=tag, score=score, target=target if isinstance(target, str) else 'given',
                    rel_err=float(err.max()), bound=bound, min_margin=float(ref.margin.min()), min_tie_gap=float(gap.min()),
                    windows=len(x), drop_scale=float(np.abs(want).max() / ref.scale.max()))
    assert np.abs(want).max() > 0, tag
    assert err.max() <= bound, '%s %s: %.3e (window %d)' % (tag, score, err.max(), int(np.argmax(err)))
    return err


@pytest.mark.parametrize('name', sorted(NETS))
def test_occlusion_against_float64(name):
    net = _model(name)
    if name == 'b':
        assert net._relabelled
    if name == 'c_maps':
        assert net._pool_maps[0] is not None
    if name == 'wide':
        assert net.layer_precisions() == ['f32', 'bf16x3']
    ref, P = _reference(name, net)
    x = _data(name)
    M, C = x.shape[1], NETS[name]['M'][-1]
    labels = np.random.RandomState(4).randint(0, C, S)
    base = 0.5 * np.random.RandomState(5).randn(M, x.shape[2]).astype(np.float32)
    bound = WIDE_REL if name == 'wide' else REL
    cases = [('cluster', None, 'logit', 'predicted'), ('holes', base, 'logprob', 'label'), ('cluster', base, 'logit', 2),
             ('holes', None, 'logit', labels[::-1].copy())]
    sets = _group_sets(M)
    if 'vertex' in sets:
        cases.append(('vertex', base, 'logprob', 'predicted'))
    for gname, baseline, score, target in cases:
        groups = sets[gname]
        drop, t = net.occlusion(x, target, score, groups, baseline, batch_size=64, labels=labels)
        _check('%s/%s' % (name, gname), net, ref, P, x, drop, t, target, score, groups, baseline, bound, labels)


def _finetuner(tmp_path, monkeypatch, tuning):
    name = 'a3'
    s = NETS[name]
    monkeypatch.setenv('CHEBGCN_HOME', str(tmp_path))
    pre = _model(name, dir_name='pre')
    pre._save_best(50.0, 7, [])
    torch.manual_seed(3)
    return models_gcn.finetuning_cgcnn({'device': DEV}, str(tmp_path) + '/checkpoints/', _laplacians(name), s['F'], s['K'],
                                       s['p'], [12, 5], channel=s['channel'], dir_name='pre', batch_size=BS, verbose=False,
                                       flag_tuning=tuning)


class FineRefNet(OccRefNet):
    """finetuning_cgcnn in float64 on an unpooled trunk: the conv layers, then the top layer's bias-ReLU output flattened as
    [S, M*F] (element m*F + f), then newfc1 ... newlogits."""

    def logits(self, P, x):
        assert all(pp == 1 for pp in self.p)
        h = x
        for i in range(len(self.p)):
            pre = self.conv(i, h, P['conv%d/weights' % (i + 1)]) + P['conv%d/bias' % (i + 1)]
            self._decision(pre.detach().numpy(), pre)
            h = torch.relu(pre)
        h = h.reshape(h.shape[0], -1)
        for i in range(len(self.M)):
            scope = 'newlogits' if i + 1 == len(self.M) else 'newfc%d' % (i + 1)
            h = h @ P[scope + '/weights'] + P[scope + '/bias']
            if i + 1 < len(self.M):
                self._decision(h.detach().numpy(), h)
                h = torch.relu(h)
        return h


@pytest.mark.parametrize('tuning', [False, True])
def test_finetuning_cgcnn_occlusion(tmp_path, monkeypatch, tuning):
    ft = _finetuner(tmp_path, monkeypatch, tuning)
    assert ft.train_layers == (['conv4', 'conv5', 'conv6'] if tuning else [])
    ref, P = _reference('a3', ft, FineRefNet)
    x = _data('a3')
    M = x.shape[1]
    labels = np.arange(S) % 5
    base = 0.5 * np.random.RandomState(5).randn(M, x.shape[2]).astype(np.float32)
    sets = _group_sets(M)
    for gname, baseline, score, target in (('cluster', None, 'logit', 'predicted'), ('holes', base, 'logprob', 'label')):
        drop, t = ft.occlusion(x, target, score, sets[gname], baseline, batch_size=32, labels=labels)
        _check('finetune%d/%s' % (tuning, gname), ft, ref, P, x, drop, t, target, score, sets[gname], baseline, REL, labels)
    maps, counts = ft.occlusion_maps(x, labels, groups=sets['cluster'], batch_size=32)
    drop, _ = ft.occlusion(x, 'label', groups=sets['cluster'], batch_size=32, labels=labels)
    assert np.array_equal(counts, np.bincount(labels, minlength=5))
    for k in range(5):
        want = drop[labels == k].astype(np.float64).mean(axis=0)
        assert np.abs(maps[k] - want).max() <= 1e-12 * np.abs(want).max(), k


@pytest.mark.parametrize('name', ['a3', 'c_max', 'b'])
def test_occlusion_maps_are_class_means_of_occlusion(name):
    net = _model(name)
    x = _data(name)
    M, C = x.shape[1], NETS[name]['M'][-1]
    labels = np.array([0, 1, 3, 0, 3, 3, 1, 0, 0, 3])         # classes 2 and 4 have no window
    for groups, score in ((_group_sets(M)['cluster'], 'logit'), (_group_sets(M)['holes'], 'logprob')):
        maps, counts = net.occlusion_maps(x, labels, score=score, groups=groups, batch_size=48)
        drop, t = net.occlusion(x, target=labels, score=score, groups=groups, batch_size=48)
        assert np.array_equal(t, labels)
        G = int(np.max(groups)) + 1
        assert maps.dtype == np.float64 and maps.shape == (C, G)
        assert counts.dtype == np.int64 and np.array_equal(counts, np.bincount(labels, minlength=C))
        d = drop.astype(np.float64)
        for k in range(C):
            if counts[k] == 0:
                assert not maps[k].any()
                continue
            want = d[labels == k].mean(axis=0)
            err = np.abs(maps[k] - want).max() / max(np.abs(want).max(), 1e-30)
            record_measured('occlusion_maps_vs_mean', net=name, score=score, cls=k, rel_err=err)
            assert err <= 1e-12, (k, err)


def test_kernels_reached():
    for name in ('a15', 'b', 'c_maps'):
        net = _model(name)
        x = _data(name)
        groups = _group_sets(x.shape[1])['cluster']
        _lib.dispatch_log = log = []
        try:
            net.occlusion(x, groups=groups, batch_size=32)
            kernels = {w: d for w, d in log}
            assert kernels['occlusion_rows'] == 'occlusion_rows_kernel'
            assert kernels['occlusion_score'] == 'occlusion_score_kernel<logit>'
            assert kernels['saliency_seed'] == 'saliency_seed_kernel<argmax>'
            assert not [d for _, d in log if 'bwd' in d or 'adam' in d], log
            del log[:]
            net.occlusion_maps(x, np.arange(S) % 3, score='logprob', groups=groups, batch_size=32)
            kernels = {w: d for w, d in log}
            assert kernels['occlusion_score'] == 'occlusion_score_kernel<logprob>'
            assert kernels['occlusion_class_sums'] == 'saliency_class_sum_kernel'
            assert 'saliency_seed' not in kernels
        finally:
            _lib.dispatch_log = None


def _boom(*a, **k):
    raise AssertionError('the occlusion pass called the vendor GEMM')


@pytest.mark.parametrize('name', ['a3', 'b', 'c_max', 'c_maps', 'fourier', 'wide'])
def test_pass_launches_no_backward_optimizer_or_gemm(name, monkeypatch):
    net = _model(name)
    x = _data(name)
    monkeypatch.setattr(torch, 'addmm', _boom)
    monkeypatch.setattr(torch, 'matmul', _boom)
    timers = ops.KernelTimers()
    monkeypatch.setattr(ops, 'timers', timers)
    groups = _group_sets(x.shape[1])['cluster']
    net.occlusion(x, score='logprob', groups=groups, batch_size=16)
    net.occlusion_maps(x, np.arange(S) % 5, groups=groups, baseline=np.ones(x.shape[1:], np.float32))
    names = list(timers.records)
    assert 'occlusion_rows' in names and 'occlusion_score' in names and 'occlusion_class_sums' in names, names
    bad = [n for n in names if 'bwd' in n or n.startswith('bias_grad') or 'adam' in n]
    assert not bad, bad


@pytest.mark.parametrize('name', ['a3', 'b', 'c_avg', 'spline'])
def test_reruns_bit_identical_and_batch_size(name):
    net = _model(name)
    x = _data(name, n=9)
    for gname, groups in _group_sets(x.shape[1]).items():
        G1 = int(np.max(groups)) + 2 if groups is not None else x.shape[1] + 1
        d1, t1 = net.occlusion(x, score='logprob', groups=groups, batch_size=32)
        d2, t2 = net.occlusion(x, score='logprob', groups=groups, batch_size=32)
        assert np.array_equal(d1, d2) and np.array_equal(t1, t2)
        scale = np.maximum(np.abs(d1).max(axis=1), 1e-30)
        # a pass ending mid-window; one whole window and a bit; several windows per pass; the model's own batch size
        for bs in (G1 // 2 + 1, G1 + 3, 3 * G1 + 1, None):
            db, tb = net.occlusion(x, score='logprob', groups=groups, batch_size=bs)
            assert np.array_equal(tb, t1)
            err = float((np.abs(db - d1).max(axis=1) / scale).max())
            record_measured('occlusion_batch_size', net=name, groups=gname, batch_size=bs, rel_err=err)
            assert err <= 1e-6, (gname, bs, err)
        m1, c1 = net.occlusion_maps(x, np.arange(9) % 5, groups=groups, batch_size=32)
        m2, c2 = net.occlusion_maps(x, np.arange(9) % 5, groups=groups, batch_size=32)
        assert np.array_equal(m1, m2) and np.array_equal(c1, c2)


class _NoDataParallel:
    capturable = True

    def __getattr__(self, name):
        raise AssertionError('the occlusion pass reached the data-parallel helper (%s)' % name)


def _state(net):
    return [t.detach().clone() for t in (net._flat, net._grad, net._adam_m, net._adam_v)] + \
        [net.global_step, float(net._loss_ema), net.training_mode]


def _same(a, b):
    return all(torch.equal(u, v) if isinstance(u, torch.Tensor) else u == v for u, v in zip(a, b))


def test_model_state_untouched_and_next_step_bit_identical():
    name = 'a3'
    x = _data(name, n=BS)
    labels = torch.as_tensor(np.arange(BS) % 5, dtype=torch.int64, device=DEV)
    nets = [_model(name, seed=7), _model(name, seed=7)]
    for net in nets:
        net.enable_step_graph(True)
        xs = net._gather(net.stage(x), torch.arange(BS, dtype=torch.int32, device=DEV))
        for _ in range(3):
            net.train_step(xs, labels)          # two eager steps, then the captured one
        assert net._sg is not None
    a, b = nets
    torch.cuda.synchronize()
    assert _same(_state(a), _state(b))
    before, sg, grad_view = _state(a), a._sg, a.gradient('conv1/weights').clone()
    groups = _group_sets(x.shape[1])['cluster']
    a._dp = _NoDataParallel()
    try:
        a.occlusion(_data(name), score='logprob', groups=groups)
        a.occlusion(_data(name), groups=_group_sets(x.shape[1])['holes'], baseline=np.ones(x.shape[1:]), batch_size=5)
        a.occlusion_maps(_data(name), np.arange(S) % 5, groups=groups)
    finally:
        a._dp = None
    torch.cuda.synchronize()
    assert _same(_state(a), before)
    assert a._sg is sg and a._step_graph_on and torch.equal(a.gradient('conv1/weights'), grad_view)
    assert a._pass is None
    for net in nets:
        xs = net._gather(net.stage(x), torch.arange(BS, dtype=torch.int32, device=DEV))
        net.train_step(xs, labels)
    torch.cuda.synchronize()
    assert _same(_state(a), _state(b))


def test_model_perf_occlusion_maps_from_fit_checkpoint(tmp_path, monkeypatch):
    name = 'a3'
    monkeypatch.setenv('CHEBGCN_HOME', str(tmp_path))
    xtr = _data(name, seed=11, n=16)
    ytr = np.arange(16) % 5
    net = _model(name, num_epochs=2, eval_frequency=2, dir_name='occ')
    net.fit(xtr, ytr, xtr[:8], ytr[:8])
    root = str(tmp_path) + '/checkpoints/occ'
    x, labels = _data(name), np.arange(S) % 5
    groups = _group_sets(x.shape[1])['cluster']
    maps, counts = models_gcn.model_perf().occlusion_maps(root, x, labels, batch_size=BS, groups=groups, score='logprob')
    live = models_gcn.model_perf._restore(root, BS, model=net)
    want, wcounts = live.occlusion_maps(x, labels, groups=groups, score='logprob')
    assert np.array_equal(maps, want) and np.array_equal(counts, wcounts)


def test_saliency_still_refuses_finetuned_models(tmp_path, monkeypatch):
    ft = _finetuner(tmp_path, monkeypatch, False)
    with pytest.raises(NotImplementedError, match='finetuning_cgcnn'):
        ft.saliency(_data('a3'))
