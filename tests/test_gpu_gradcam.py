"""Grad-CAM maps (base_model.gradcam / gradcam_maps, model_perf.gradcam_maps) on the MI355X against the float64 restatement of
tests/test_gradcam_host.py, on the networks of tests/test_gpu_saliency.py -- the atlas shape at channel 3 and 15, a relabelled
graph of more than 1024 vertices, pooled networks (through index maps too), fourier, spline and split bf16 -- every layer of a
pooled network and the top plus a lower layer of the others, and on finetuning_cgcnn with a frozen and with a tuned trunk.
Also: the per-class maps, the kernels a call names, what it must not launch, where the input gradient stops, bit-identical
reruns, batch-size invariance, the model's state and checkpoints."""

import numpy as np
import pytest
import torch

from conftest import record_measured
from gcn_fmri_decoding_amd import _lib, models_gcn, ops
from test_gpu_occlusion import FineRefNet, _finetuner
from test_gpu_saliency import BS, NETS, REL, S, WIDE_REL, _data, _laplacians, _model
from test_gradcam_host import CamRefNet

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
CASES = [('gradcam', 'logit', 'predicted', True), ('grad_x_activation', 'logprob', 'labels', False),
         ('gradcam', 'logprob', 'labels', False), ('grad_x_activation', 'logit', 'predicted', True)]


def _reference(name, net, head='mean'):
    s = NETS[name]
    ref = CamRefNet(_laplacians(name), s['F'], s['K'], s['p'], s['M'], s.get('filter', 'chebyshev5'), s.get('brelu', 'b1relu'),
                    s.get('pool', 'mpool1'))
    ref.head = head
    P = {n: torch.as_tensor(net.variable(n).detach().cpu().numpy().astype(np.float64)) for n in net.variables()}
    return ref, P


def _layers(name):
    nl = len(NETS[name]['p'])
    return list(range(nl)) if name == 'c_max' else [0, nl - 1]


def _check(tag, net, ref, P, x, layer, labels, bound, margin_floor):
    """Every case of CASES at one layer against the float64 restatement.  The error of a window is relative to the scale of
    its map's terms (CamRefNet.scale): in 'gradcam' the mean of G over the vertices may cancel, and then the map is far smaller
    than the fp32 rounding of the gradient it is formed from; the error relative to the map itself is recorded as well."""
    for method, score, tgt, relu in CASES:
        target = 'predicted' if tgt == 'predicted' else labels
        cam, t = net.gradcam(x, 'conv%d' % (layer + 1), target, score, method, relu)
        want, want_t, _ = ref.gradcam(P, x, layer, target, score, method, relu)
        margin, scale = ref.margin, ref.scale
        assert cam.dtype == np.float32 and cam.shape == x.shape[:2] and t.dtype == np.int64
        assert np.array_equal(t, want_t), (tag, method, score, t, want_t)
        assert scale.min() > 0, tag
        # A window whose float64 forward has a ReLU or max-pool decision within the reach of the arithmetic under test is not
        # held to the bound: the GPU may take the other branch there.  At least three of the ten windows must be held to it.
        keep = margin > margin_floor
        diff = np.abs(cam.astype(np.float64) - want).max(axis=1)
        err = diff / scale
        of_map = diff / np.maximum(np.abs(want).max(axis=1), 1e-30)
        record_measured('gradcam_vs_float64', case=tag, layer=layer + 1, method=method, score=score, target=tgt, relu=relu,
                        rel_err=float(err[keep].max()), bound=bound, windows=int(keep.sum()), all_windows_err=float(err.max()),
                        of_map_err=float(of_map[keep].max()), min_margin=float(margin.min()))
        assert keep.sum() >= 3, (tag, method, score, margin)
        assert err[keep].max() <= bound, '%s conv%d %s %s: %.3e' % (tag, layer + 1, method, score, err[keep].max())


@pytest.mark.parametrize('name', sorted(NETS))
def test_gradcam_against_float64(name):
    net = _model(name)
    if name == 'b':
        assert net._relabelled
    if name == 'c_maps':
        assert net._pool_maps[0] is not None
    if name == 'wide':
        assert net.layer_precisions() == ['f32', 'bf16x3']
    ref, P = _reference(name, net)
    x = _data(name)
    labels = np.random.RandomState(4).randint(0, NETS[name]['M'][-1], S)
    wide = name == 'wide'
    for layer in _layers(name):
        _check(name, net, ref, P, x, layer, labels, WIDE_REL if wide else REL, 1e-5 if wide else 1e-6)


@pytest.mark.parametrize('tuning', [False, True])
def test_finetuning_cgcnn_gradcam(tmp_path, monkeypatch, tuning):
    ft = _finetuner(tmp_path, monkeypatch, tuning)
    assert ft.train_layers == (['conv4', 'conv5', 'conv6'] if tuning else [])
    ref, P = _reference('a3', ft, head='flat')
    x = _data('a3')
    fine = FineRefNet(_laplacians('a3'), NETS['a3']['F'], NETS['a3']['K'], NETS['a3']['p'], [12, 5])
    with torch.no_grad():                           # the restatement's flat head is the occlusion test's
        z, zf = ref.logits(P, torch.as_tensor(x.astype(np.float64))), fine.logits(P, torch.as_tensor(x.astype(np.float64)))
    assert torch.allclose(z, zf, rtol=1e-12, atol=0)
    labels = np.arange(S) % 5
    for layer in (5, 2):                            # the top layer before its pooling, and one below the tuned ones
        _check('finetune%d' % tuning, ft, ref, P, x, layer, labels, REL, 1e-6)
    maps, counts = ft.gradcam_maps(x, labels, layer='conv6', method='grad_x_activation')
    cam, _ = ft.gradcam(x, None, labels, method='grad_x_activation')
    assert np.array_equal(counts, np.bincount(labels, minlength=5))
    for k in range(5):
        want = cam[labels == k].astype(np.float64).mean(axis=0)
        assert np.abs(maps[k] - want).max() <= 1e-12 * np.abs(want).max(), k
    with pytest.raises(NotImplementedError, match='finetuning_cgcnn'):
        ft.saliency(x)


@pytest.mark.parametrize('name', ['a3', 'c_max', 'b'])
def test_gradcam_maps_are_class_means_of_gradcam(name):
    net = _model(name)
    x = _data(name)
    M, C = x.shape[1], NETS[name]['M'][-1]
    labels = np.array([0, 1, 3, 0, 3, 3, 1, 0, 0, 3])         # classes 2 and 4 have no window
    for layer, score, method in (('conv1', 'logit', 'gradcam'), (None, 'logprob', 'grad_x_activation')):
        maps, counts = net.gradcam_maps(x, labels, layer=layer, score=score, method=method)
        cam, t = net.gradcam(x, layer, labels, score, method)
        assert np.array_equal(t, labels)
        assert maps.dtype == np.float64 and maps.shape == (C, M)
        assert counts.dtype == np.int64 and np.array_equal(counts, np.bincount(labels, minlength=C))
        d = cam.astype(np.float64)
        for k in range(C):
            if counts[k] == 0:
                assert not maps[k].any()
                continue
            want = d[labels == k].mean(axis=0)
            err = np.abs(maps[k] - want).max() / max(np.abs(want).max(), 1e-30)
            record_measured('gradcam_maps_vs_mean', net=name, layer=layer, score=score, cls=k, rel_err=err)
            assert err <= 1e-12, (k, err)


def test_kernels_reached_and_the_gradient_stops_at_the_layer():
    """The new kernels by name; and at layer l the pass runs the input gradients of the layers above l only: the atlas
    network's fused layers name one chebgcn_fused_layer_bwd_x per layer above l and pass (none at the top layer, so layer 1's
    at Fin = channel never runs), and the index-map pooling of c_maps' layer 1 (output of conv1) never runs backward."""
    x = _data('a15')
    net = _model('a15')
    passes = -(-S // BS)
    _lib.dispatch_log = log = []
    try:
        for li in (5, 2, 0):
            del log[:]
            net.gradcam(x, 'conv%d' % (li + 1), score='logprob')
            kernels = {w: d for w, d in log}
            assert kernels['gradcam_weights'] == 'gradcam_weights_kernel'
            assert kernels['gradcam_map'] == 'gradcam_map_kernel<gradcam>'
            assert kernels['saliency_seed'] == 'saliency_seed_kernel<argmax>'
            assert [w for w, _ in log].count('fused_layer_bwd_x') == passes * (5 - li), (li, log)
            assert not [d for _, d in log if 'bwd_w' in d or 'adam' in d or 'bias_grad' in d], log
        del log[:]
        net.gradcam_maps(x, np.arange(S) % 3, layer='conv4', method='grad_x_activation')
        kernels = {w: d for w, d in log}
        assert kernels['gradcam_map'] == 'gradcam_map_kernel<grad_x_activation>'
        assert kernels['saliency_seed'] == 'saliency_seed_kernel<target>'
        assert kernels['occlusion_class_sums'] == 'saliency_class_sum_kernel'
        assert 'gradcam_weights' not in kernels
        net = _model('c_maps')
        for layer in ('conv1', 'conv2'):
            del log[:]
            net.gradcam(_data('c_maps'), layer)
            names = [w for w, _ in log]
            assert 'gradcam_map' in names and 'pool_scatter_bwd' not in names, (layer, names)
    finally:
        _lib.dispatch_log = None


def _boom(*a, **k):
    raise AssertionError('the gradcam pass called the vendor GEMM')


@pytest.mark.parametrize('name', ['a3', 'b', 'c_max', 'c_maps', 'fourier', 'wide'])
def test_pass_launches_no_weight_gradient_bias_gradient_optimizer_or_gemm(name, monkeypatch):
    net = _model(name)
    x = _data(name)
    monkeypatch.setattr(torch, 'addmm', _boom)
    monkeypatch.setattr(torch, 'matmul', _boom)
    timers = ops.KernelTimers()
    monkeypatch.setattr(ops, 'timers', timers)
    net.gradcam(x, 'conv1', score='logprob')
    net.gradcam(x, method='grad_x_activation', relu=False)
    net.gradcam_maps(x, np.arange(S) % 5, layer='conv1')
    names = list(timers.records)
    assert 'gradcam_map' in names and 'gradcam_weights' in names and 'fc_bwd_x' in names, names
    bad = [n for n in names if 'bwd_w' in n or n.startswith('bias_grad') or 'adam' in n or 'nadam' in n]
    assert not bad, bad


def test_finetuning_pass_launches_no_weight_gradient_or_gemm(tmp_path, monkeypatch):
    ft = _finetuner(tmp_path, monkeypatch, True)
    x = _data('a3')
    monkeypatch.setattr(torch, 'addmm', _boom)
    monkeypatch.setattr(torch, 'matmul', _boom)
    _lib.dispatch_log = log = []
    try:
        ft.gradcam(x, 'conv4')
        ft.gradcam(x, method='grad_x_activation')
    finally:
        _lib.dispatch_log = None
    names = [w for w, _ in log]
    assert 'gradcam_map' in names and 'fc_bwd' in names, names
    assert not [d for _, d in log if 'bwd_w' in d or 'adam' in d or 'bias_grad' in d], log
    before = ft._grad.clone()
    ft.gradcam(x, 'conv5')
    assert torch.equal(ft._grad, before)


@pytest.mark.parametrize('name', ['a3', 'b', 'c_avg', 'spline'])
def test_reruns_bit_identical_and_batch_size(name):
    net = _model(name)
    x = _data(name, n=9)
    for layer, method in (('conv1', 'gradcam'), (None, 'grad_x_activation')):
        c1, t1 = net.gradcam(x, layer, method=method, relu=False)
        c2, t2 = net.gradcam(x, layer, method=method, relu=False)
        assert np.array_equal(c1, c2) and np.array_equal(t1, t2)
        scale = np.abs(c1).max(axis=1)
        for bs in (1, 7, 16):                       # one window per pass; a padded last batch; all in one padded pass
            cb, tb = net.gradcam(x, layer, method=method, relu=False, batch_size=bs)
            assert np.array_equal(tb, t1)
            err = float((np.abs(cb - c1).max(axis=1) / scale).max())
            record_measured('gradcam_batch_size', net=name, layer=layer, method=method, batch_size=bs, rel_err=err)
            assert err <= 2 * REL, (bs, err)
        m1, k1 = net.gradcam_maps(x, np.arange(9) % 5, layer=layer, method=method)
        m2, k2 = net.gradcam_maps(x, np.arange(9) % 5, layer=layer, method=method)
        assert np.array_equal(m1, m2) and np.array_equal(k1, k2)


class _NoDataParallel:
    capturable = True

    def __getattr__(self, name):
        raise AssertionError('the gradcam pass reached the data-parallel helper (%s)' % name)


def _state(net):
    return [t.detach().clone() for t in (net._flat, net._grad, net._adam_m, net._adam_v)] + \
        [net.global_step, float(net._loss_ema), net.training_mode, net.fuse_feature_mean]


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
    a._dp = _NoDataParallel()
    try:
        a.gradcam(_data(name), score='logprob')
        a.gradcam(_data(name), 'conv3', method='grad_x_activation', batch_size=5)
        a.gradcam_maps(_data(name), np.arange(S) % 5, layer='conv1')
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


def test_model_perf_gradcam_maps_from_fit_checkpoint(tmp_path, monkeypatch):
    name = 'a3'
    monkeypatch.setenv('CHEBGCN_HOME', str(tmp_path))
    xtr = _data(name, seed=11, n=16)
    ytr = np.arange(16) % 5
    net = _model(name, num_epochs=2, eval_frequency=2, dir_name='cam')
    net.fit(xtr, ytr, xtr[:8], ytr[:8])
    root = str(tmp_path) + '/checkpoints/cam'
    x, labels = _data(name), np.arange(S) % 5
    maps, counts = models_gcn.model_perf().gradcam_maps(root, x, labels, batch_size=BS, layer='conv2', score='logprob')
    live = models_gcn.model_perf._restore(root, BS, model=net)
    want, wcounts = live.gradcam_maps(x, labels, layer='conv2', score='logprob')
    assert np.array_equal(maps, want) and np.array_equal(counts, wcounts)
