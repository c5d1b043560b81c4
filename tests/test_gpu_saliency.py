"""Saliency maps (cgcnn.saliency / saliency_maps, model_perf.saliency_maps) on the MI355X against the float64 restatement of
tests/test_saliency_host.py, on every path cgcnn trains: (a) the atlas shape, six fused layers, at channel 3 and 15 (layer 1's
fused input gradient at Fin = channel), (b) a graph of more than 1024 vertices in relabelled vertex order, (c) pooled networks
(b2relu with mpool1 / apool1; and pooling through index maps out of a relabelled level), (d) fourier and spline, (e) a layer
of more than 32 filters under contraction='auto' (split bf16).  Also: the per-class maps, the kernels every pass names, what a
pass must not launch, bit-identical reruns, batch-size invariance, the model's state, checkpoints and the fine-tuning refusal."""

import numpy as np
import pytest
import torch

from conftest import record_measured
from gcn_fmri_decoding_amd import _lib, graph, models_gcn, ops
from test_saliency_host import RefNet

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
S, BS = 10, 4               # windows, batch size (the last batch is padded)
REL = 1e-5
NETS = {
    'a3': dict(N=360, levels=0, F=[16] * 6, K=[4] * 6, p=[1] * 6, M=[12, 5], channel=3),
    'a15': dict(N=360, levels=0, F=[16] * 6, K=[4] * 6, p=[1] * 6, M=[12, 5], channel=15, brelu='b2relu'),
    'b': dict(N=1200, levels=1, F=[6, 8], K=[4, 3], p=[1, 1], M=[9, 5], channel=2, brelu='b2relu'),
    'c_max': dict(N=100, levels=2, F=[4, 5, 6], K=[3, 3, 2], p=[1, 2, 2], M=[9, 5], channel=2, brelu='b2relu', pool='mpool1'),
    'c_avg': dict(N=100, levels=2, F=[4, 5, 6], K=[3, 3, 2], p=[1, 2, 2], M=[9, 5], channel=2, brelu='b2relu', pool='apool1'),
    'c_maps': dict(N=1200, levels=1, F=[4, 6], K=[3, 3], p=[2, 1], M=[9, 5], channel=2, brelu='b2relu', pool='mpool1'),
    'fourier': dict(N=100, levels=0, F=[4, 5], K=[1, 1], p=[1, 1], M=[9, 5], channel=2, filter='fourier'),
    'spline': dict(N=100, levels=0, F=[4, 5], K=[5, 4], p=[1, 1], M=[9, 5], channel=2, filter='spline', brelu='b2relu'),
    'wide': dict(N=32, levels=0, F=[64, 64], K=[5, 5], p=[1, 1], M=[12, 5], channel=3, contraction='auto'),
}
WIDE_REL = 1e-4             # (e): split bf16 (3e-6 ... 6e-6 of a layer's scale per contraction) through two layers and back
_graphs = {}


def _laplacians(name):
    s = NETS[name]
    key = (s['N'], s['levels'])
    if key not in _graphs:
        _graphs[key] = graph.synthetic_graph(s['N'], k=6, levels=s['levels'], seed=3)[0]
    Ls = _graphs[key]
    return Ls + [Ls[-1]] * max(0, len(s['p']) - len(Ls))


def _model(name, seed=0, **kw):
    s = NETS[name]
    torch.manual_seed(seed)
    args = dict(channel=s['channel'], brelu=s.get('brelu', 'b1relu'), pool=s.get('pool', 'mpool1'),
                filter=s.get('filter', 'chebyshev5'), batch_size=BS, verbose=False)
    args.update(kw)
    net = models_gcn.cgcnn({'device': DEV}, _laplacians(name), s['F'], s['K'], s['p'], s['M'], **args)
    net.contraction = s.get('contraction', 'f32')
    return net


def _data(name, seed=1, n=S):
    s = NETS[name]
    rs = np.random.RandomState(seed)
    return rs.randn(n, _laplacians(name)[0].shape[0], s['channel']).astype(np.float32)


def _reference(name, net):
    s = NETS[name]
    ref = RefNet(_laplacians(name), s['F'], s['K'], s['p'], s['M'], s.get('filter', 'chebyshev5'), s.get('brelu', 'b1relu'),
                 s.get('pool', 'mpool1'))
    P = {n: torch.as_tensor(net.variable(n).detach().cpu().numpy().astype(np.float64)) for n in net.variables()}
    return ref, P


def _per_window_err(got, ref, keep=None):
    d = np.abs(got.astype(np.float64) - ref).reshape(len(ref), -1).max(axis=1)
    e = d / np.maximum(np.abs(ref).reshape(len(ref), -1).max(axis=1), 1e-30)
    return float(e[keep].max() if keep is not None else e.max())


CASES = [('gradient', 'logit', 'predicted'), ('gradient', 'logprob', 'labels'), ('grad_x_input', 'logit', 'labels'),
         ('grad_x_input', 'logprob', 'predicted'), ('integrated', 'logit', 'predicted'), ('integrated', 'logprob', 'labels')]


@pytest.mark.parametrize('name', sorted(NETS))
def test_saliency_against_float64(name):
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
    base = 0.5 * np.random.RandomState(5).randn(*x.shape[1:]).astype(np.float32)
    bound = WIDE_REL if name == 'wide' else REL
    for method, score, tgt in CASES:
        target = 'predicted' if tgt == 'predicted' else labels
        baseline = base if score == 'logprob' else None
        attr, t = net.saliency(x, target, score, method, steps=6, baseline=baseline)
        want, want_t = ref.saliency(P, x, target, score, method, 6, baseline)
        assert attr.dtype == np.float32 and attr.shape == x.shape and t.dtype == np.int64
        assert np.array_equal(t, want_t), (method, score, t, want_t)
        # A window whose float64 forward (at any point of the path) has a ReLU or max-pool decision within the reach of the
        # arithmetic under test (1e-6 of the layer's scale in fp32, 1e-5 with split bf16) is not held to the bound: the GPU may
        # take the other branch there.  At least three of the ten windows must be held to it; all are recorded.
        keep = ref.margin > (1e-5 if name == 'wide' else 1e-6)
        err = _per_window_err(attr, want, keep)
        record_measured('saliency_vs_float64', net=name, method=method, score=score, rel_err=err, bound=bound,
                        windows=int(keep.sum()), all_windows_err=_per_window_err(attr, want), min_margin=float(ref.margin.min()))
        assert keep.sum() >= 3, (name, method, score, ref.margin)
        assert err <= bound, '%s %s %s: %.3e' % (name, method, score, err)


@pytest.mark.parametrize('name', ['a3', 'c_max'])
@pytest.mark.parametrize('method', ['gradient', 'integrated'])
def test_saliency_maps_are_class_means_of_saliency(name, method):
    net = _model(name)
    x = _data(name)
    labels = np.array([0, 1, 3, 0, 3, 3, 1, 0, 0, 3])         # classes 2 and 4 have no window
    C = NETS[name]['M'][-1]
    for absolute in (False, True):
        maps, counts = net.saliency_maps(x, labels, absolute=absolute, method=method, steps=5)
        attr, t = net.saliency(x, target=labels, method=method, steps=5)
        assert np.array_equal(t, labels)
        a = np.abs(attr.astype(np.float64)) if absolute else attr.astype(np.float64)
        assert maps.dtype == np.float64 and maps.shape == (C,) + x.shape[1:]
        assert counts.dtype == np.int64 and np.array_equal(counts, np.bincount(labels, minlength=C))
        for k in range(C):
            if counts[k] == 0:
                assert not maps[k].any()
                continue
            want = a[labels == k].mean(axis=0)
            err = np.abs(maps[k] - want).max() / max(np.abs(want).max(), 1e-30)
            record_measured('saliency_maps_vs_mean', net=name, method=method, absolute=absolute, cls=k, rel_err=err)
            assert err <= 1e-6, (k, err)


def test_kernels_reached():
    for name, layer1 in (('a15', 'fused_layer_bwd_x'), ('b', None), ('c_maps', 'pool_scatter_bwd')):
        net = _model(name)
        x = _data(name)
        _lib.dispatch_log = log = []
        try:
            net.saliency(x, method='integrated', steps=3)
            names = [w for w, _ in log]
            kernels = {w: d for w, d in log}
            assert kernels['saliency_seed'] in ('saliency_seed_kernel<argmax>', 'saliency_seed_kernel<target>')
            assert kernels['saliency_path'] == 'saliency_path_kernel'
            assert kernels['saliency_reduce'] == 'saliency_rows_kernel'
            assert 'saliency_seed_kernel<argmax>' in [d for w, d in log if w == 'saliency_seed']
            if layer1:
                assert layer1 in names, names
            del log[:]
            net.saliency_maps(x, np.arange(S) % 3)
            kernels = {w: d for w, d in log}
            assert kernels['saliency_seed'] == 'saliency_seed_kernel<target>'
            assert kernels['saliency_reduce'] == 'saliency_rows_kernel + saliency_class_sum_kernel'
            assert 'saliency_path' not in kernels
        finally:
            _lib.dispatch_log = None


def _boom(*a, **k):
    raise AssertionError('the saliency pass called the vendor GEMM')


@pytest.mark.parametrize('name', ['a3', 'b', 'c_max', 'c_maps', 'fourier', 'wide'])
def test_pass_launches_no_weight_gradient_bias_gradient_optimizer_or_gemm(name, monkeypatch):
    net = _model(name)
    x = _data(name)
    monkeypatch.setattr(torch, 'addmm', _boom)
    monkeypatch.setattr(torch, 'matmul', _boom)
    timers = ops.KernelTimers()
    monkeypatch.setattr(ops, 'timers', timers)
    net.saliency(x, score='logprob')
    net.saliency(x, method='integrated', steps=3)
    net.saliency_maps(x, np.arange(S) % 5, absolute=True, method='grad_x_input')
    names = list(timers.records)
    assert 'saliency_reduce' in names and 'saliency_seed' in names and 'fc_bwd_x' in names, names
    bad = [n for n in names if 'bwd_w' in n or n.startswith('bias_grad') or 'adam' in n or 'nadam' in n]
    assert not bad, bad


@pytest.mark.parametrize('name', ['a3', 'b', 'c_avg'])
def test_reruns_bit_identical_and_batch_size(name):
    net = _model(name)
    x = _data(name, n=9)
    for method in ('gradient', 'integrated'):
        a1, t1 = net.saliency(x, method=method, steps=4)
        a2, t2 = net.saliency(x, method=method, steps=4)
        assert np.array_equal(a1, a2) and np.array_equal(t1, t2)
        scale = np.abs(a1).reshape(len(x), -1).max(axis=1)
        for bs in (1, 7, 16):
            ab, tb = net.saliency(x, method=method, steps=4, batch_size=bs)
            assert np.array_equal(tb, t1)
            err = float((np.abs(ab - a1).reshape(len(x), -1).max(axis=1) / scale).max())
            record_measured('saliency_batch_size', net=name, method=method, batch_size=bs, rel_err=err)
            assert err <= 2 * REL, (bs, err)
        m1, c1 = net.saliency_maps(x, np.arange(9) % 5, method=method, steps=4)
        m2, c2 = net.saliency_maps(x, np.arange(9) % 5, method=method, steps=4)
        assert np.array_equal(m1, m2) and np.array_equal(c1, c2)


class _NoDataParallel:
    capturable = True

    def __getattr__(self, name):
        raise AssertionError('the saliency pass reached the data-parallel helper (%s)' % name)


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
    a._dp = _NoDataParallel()
    try:
        a.saliency(_data(name), score='logprob')
        a.saliency(_data(name), method='integrated', steps=3, batch_size=5)
        a.saliency_maps(_data(name), np.arange(S) % 5, absolute=True)
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


def test_model_perf_saliency_maps_from_fit_checkpoint(tmp_path, monkeypatch):
    name = 'a3'
    monkeypatch.setenv('CHEBGCN_HOME', str(tmp_path))
    xtr = _data(name, seed=11, n=16)
    ytr = np.arange(16) % 5
    net = _model(name, num_epochs=2, eval_frequency=2, dir_name='sal')
    net.fit(xtr, ytr, xtr[:8], ytr[:8])
    root = str(tmp_path) + '/checkpoints/sal'
    x, labels = _data(name), np.arange(S) % 5
    maps, counts = models_gcn.model_perf().saliency_maps(root, x, labels, batch_size=BS, method='integrated', steps=3)
    live = models_gcn.model_perf._restore(root, BS, model=net)
    want, wcounts = live.saliency_maps(x, labels, method='integrated', steps=3)
    assert np.array_equal(maps, want) and np.array_equal(counts, wcounts)


def test_finetuning_cgcnn_refuses(tmp_path, monkeypatch):
    name = 'a3'
    s = NETS[name]
    monkeypatch.setenv('CHEBGCN_HOME', str(tmp_path))
    pre = _model(name, dir_name='pre')
    pre._save_best(50.0, 7, [])
    ft = models_gcn.finetuning_cgcnn({'device': DEV}, str(tmp_path) + '/checkpoints/', _laplacians(name), s['F'], s['K'],
                                     s['p'], [12, 5], channel=s['channel'], dir_name='pre', batch_size=BS, verbose=False)
    with pytest.raises(NotImplementedError, match='finetuning_cgcnn'):
        ft.saliency(_data(name))
    with pytest.raises(NotImplementedError, match='finetuning_cgcnn'):
        ft.saliency_maps(_data(name), np.arange(S) % 5)


@pytest.mark.parametrize('name', ['a3', 'b', 'c_max', 'c_maps', 'fourier', 'wide'])
def test_pass_keeps_no_weight_gradient_operand(name):
    """The forward of a saliency pass keeps what the input gradients read (masks, selection bytes, outputs) and not the
    operands of the weight gradients: no layer's Chebyshev stack [K, B, Fin, Mp] (the only four-dimensional tensors), no
    spectral layer's analysed input [B, Fin, Mp] at Fin = channel (the planes a layer-1 weight gradient would read)."""
    net = _model(name)
    x = _data(name)
    saved = []

    def pack(t):
        saved.append(tuple(t.shape))
        return t
    with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
        net.saliency(x, method='integrated', steps=2)
    assert saved
    assert not [sh for sh in saved if len(sh) == 4], saved
    if NETS[name].get('filter') in ('fourier', 'spline'):
        C, Mp = NETS[name]['channel'], ops.plane_stride(x.shape[1])
        assert not [sh for sh in saved if sh[1:] == (C, Mp)], saved
    # the training step still keeps them (its weight gradients read them)
    saved.clear()
    xs = net._gather(net.stage(x[:BS]), torch.arange(BS, dtype=torch.int32, device=DEV))
    with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
        net.train_step(xs, torch.zeros(BS, dtype=torch.int64, device=DEV))
    if NETS[name].get('filter') in ('fourier', 'spline'):
        assert [sh for sh in saved if sh[1:] == (C, Mp)], saved
    else:
        assert [sh for sh in saved if len(sh) == 4], saved


def test_label_target_takes_labels():
    net = _model('a3')
    x, labels = _data('a3'), np.arange(S) % 5
    a1, t1 = net.saliency(x, target='label', labels=labels)
    a2, t2 = net.saliency(x, target=labels)
    assert np.array_equal(a1, a2) and np.array_equal(t1, labels) and np.array_equal(t2, labels)
