"""``finetuning_cgcnn`` (lib_new/models_gcn.py:685-933) on the MI355X: the trunk restored from a cgcnn checkpoint, the logits
and one step's gradients against a float64 restatement (oracle/layers_ref.py), the Nadam kernel against float64 Nadam, gradient
descent at momentum 0, the captured step against the eager one, fit() / model_perf.predict, and the kernels every step names.
Three trunks: (a) the atlas shape (360 vertices, six layers), (b) a graph of more than 1024 vertices (relabelled vertex order),
(c) a trunk whose last layer pools (the head reads its values before the pooling)."""
import os
import shutil

import numpy as np
import pytest
import torch

from conftest import record_measured
from gcn_fmri_decoding_amd import _lib, graph, models_gcn, ops
from gcn_fmri_decoding_amd._lib import plane_stride
from oracle import layers_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
B = 8
SHAPES = {
    'a': dict(N=360, levels=0, F=[16] * 6, K=[4] * 6, p=[1] * 6, channel=3, brelu='b1relu', pool='mpool1'),
    'b': dict(N=1200, levels=1, F=[6, 8], K=[4, 3], p=[1, 1], channel=2, brelu='b2relu', pool='mpool1'),
    'c': dict(N=100, levels=2, F=[4, 5, 6], K=[3, 3, 2], p=[1, 2, 2], channel=2, brelu='b2relu', pool='apool1'),
}
HEAD = [12, 8, 5]        # widths the library's small FC kernels serve (row strides of 4 floats)
_graphs = {}
B1, B2 = float(np.float32(0.9)), float(np.float32(0.999))        # the kernel's betas are fp32


def _laplacians(shape):
    if shape not in _graphs:
        s = SHAPES[shape]
        _graphs[shape] = graph.synthetic_graph(s['N'], k=6, levels=s['levels'], seed=3)[0]
    return _graphs[shape]


def _pretrained(home, shape, seed=0):
    """A cgcnn of the given trunk, drawn at random, saved as fit() saves it under ``<home>/checkpoints/pre/model``."""
    s = SHAPES[shape]
    torch.manual_seed(seed)
    os.environ['CHEBGCN_HOME'] = str(home)
    try:
        net = models_gcn.cgcnn({'device': DEV}, _laplacians(shape), s['F'], s['K'], s['p'], [9, 5], channel=s['channel'],
                               brelu=s['brelu'], pool=s['pool'], dir_name='pre', verbose=False)
        net.contraction = 'f32'
        best = []
        net._save_best(50.0, 7, best)
    finally:
        del os.environ['CHEBGCN_HOME']
    return str(home) + '/checkpoints/', net


def _finetuner(root, shape, seed=1, **kw):
    s = SHAPES[shape]
    torch.manual_seed(seed)
    args = dict(channel=s['channel'], dir_name='pre', verbose=False, regularization=1e-3, batch_size=B)
    args.update(kw)
    net = models_gcn.finetuning_cgcnn({'device': DEV}, root, _laplacians(shape), s['F'], s['K'], s['p'], HEAD, **args)
    net.contraction = 'f32'
    return net


def _batch(net, shape, seed=2):
    rs = np.random.RandomState(seed)
    x = rs.randn(B, _laplacians(shape)[0].shape[0], SHAPES[shape]['channel']).astype(np.float32)
    y = rs.randint(0, HEAD[-1], B)
    dev_x = net.stage(x)
    return x.astype(np.float64), y, net._gather(dev_x, torch.arange(B, dtype=torch.int32, device=DEV)), \
        torch.as_tensor(y, dtype=torch.int64, device=DEV)


def _vars(net):
    return {n: net.variable(n).detach().cpu().numpy().astype(np.float64) for n in net.variables()}


def _reference(net, P, x, labels):
    """float64 forward and backward of the fine-tuning network; returns (logits, loss, grads by name)."""
    s = SHAPES[net._shape]
    Ls = [net.L[i] for i in range(len(net.p))]
    nl = len(net.p)
    cache, h = [], x
    for i in range(nl):
        W, b = P['conv%d/weights' % (i + 1)], P['conv%d/bias' % (i + 1)]
        y, T = R.chebyshev5_fwd(h, Ls[i], W, net.K[i], return_stack=True)
        a = R.brelu_fwd(y, b)
        arg = None
        if i + 1 < nl and net.p[i] > 1:
            if s['pool'] == 'mpool1':
                o, arg = R.mpool1_fwd(a, net.p[i])
            else:
                o = R.apool1_fwd(a, net.p[i])
        else:
            o = a
        cache.append((h, T, a, arg))
        h = o
    N, M, F = h.shape
    acts = [h.reshape(N, M * F)]
    nh = len(net.M)
    names = ['newfc%d' % (j + 1) for j in range(nh - 1)] + ['newlogits']
    for j, name in enumerate(names):
        acts.append(R.fc_fwd(acts[-1], P[name + '/weights'], P[name + '/bias'], relu=j + 1 < nh))
    logits = acts[-1]
    ce, d = R.softmax_xent(logits, labels)
    G = {}
    for j in reversed(range(nh)):
        name = names[j]
        d, G[name + '/weights'], G[name + '/bias'] = R.fc_bwd(d, acts[j], P[name + '/weights'], acts[j + 1], relu=j + 1 < nh)
    d = d.reshape(N, M, F)
    for i in reversed(range(max(net._lowest, 0), nl)):
        h_in, T, a, arg = cache[i]
        if i + 1 < nl and net.p[i] > 1:
            if s['pool'] == 'mpool1':
                d = R.mpool1_bwd(d, arg, net.p[i], a.shape[1])
            else:
                d = np.repeat(d / net.p[i], net.p[i], axis=1)
        d, db = R.brelu_bwd(d, a, P['conv%d/bias' % (i + 1)].shape)
        dx, dW = R.chebyshev5_bwd(d, Ls[i], P['conv%d/weights' % (i + 1)], net.K[i], T, need_dx=i > net._lowest)
        if 'conv%d' % (i + 1) in net.train_layers:
            G['conv%d/weights' % (i + 1)], G['conv%d/bias' % (i + 1)] = dW, db
        d = dx
    reg = sum(0.5 * np.sum(P[n] ** 2) for n in net.regularizers)
    return logits, ce + net.regularization * reg, G


def _rel(got, ref):
    return np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-30)


@pytest.fixture
def home(tmp_path):
    return tmp_path


def test_planes_rows_gather_and_adjoint():
    rs = np.random.RandomState(0)
    for M, F in ((360, 32), (1100, 6), (37, 40)):
        Mp = plane_stride(M)
        order = rs.permutation(M).astype(np.int32)
        planes = torch.full((3, F, Mp), float('nan'), device=DEV)
        planes[:, :, :M] = torch.as_tensor(rs.randn(3, F, M).astype(np.float32), device=DEV)
        od = torch.as_tensor(order, device=DEV)
        rows = ops.planes_to_rows(planes, M, od)
        assert _lib.last_dispatch() == 'planes_rows_kernel<to_rows>'
        ref = np.empty((3, M, F), np.float32)
        ref[:, order, :] = planes[:, :, :M].cpu().numpy().transpose(0, 2, 1)
        assert np.array_equal(rows[:, :M * F].cpu().numpy(), ref.reshape(3, M * F))
        back = ops.rows_to_planes(rows, M, F, od)
        assert _lib.last_dispatch() == 'planes_rows_kernel<to_planes>'
        assert torch.equal(back[:, :, :M], planes[:, :, :M]) and bool((back[:, :, M:] == 0).all())
        ident = ops.planes_to_rows(planes, M, None)
        assert np.array_equal(ident[:, :M * F].cpu().numpy(), planes[:, :, :M].cpu().numpy().transpose(0, 2, 1).reshape(3, -1))


def test_restore_from_cgcnn_fit_checkpoint(home, monkeypatch):
    """A cgcnn pretrained by fit(); the trunk of the fine-tuning model is its checkpoint, bit for bit."""
    s = SHAPES['c']
    monkeypatch.setenv('CHEBGCN_HOME', str(home / 'pre_home'))
    rs = np.random.RandomState(5)
    M0 = _laplacians('c')[0].shape[0]
    xtr, ytr = rs.randn(24, M0, 2).astype(np.float32), rs.randint(0, 5, 24)
    np.random.seed(0)
    torch.manual_seed(0)
    pre = models_gcn.cgcnn({'device': DEV}, _laplacians('c'), s['F'], s['K'], s['p'], [9, 5], channel=2, brelu=s['brelu'],
                           pool=s['pool'], batch_size=B, num_epochs=2, eval_frequency=2, dir_name='pre', verbose=False)
    pre.fit(xtr, ytr, xtr[:10], ytr[:10])
    root = str(home / 'pre_home') + '/checkpoints/'
    path = root + 'pre/model/'
    lines = [l.rstrip('\n').split('"')[1] for l in open(path + 'checkpoint')]
    assert lines[0] != lines[1]
    monkeypatch.setenv('CHEBGCN_HOME', str(home / 'ft_home'))
    for fallback in (False, True):
        if fallback:
            os.remove(path + lines[0] + '.pt')          # line 1 names a file that is gone: line 2 is read
            want = lines[1]
        else:
            want = lines[0]
        sd = torch.load(path + want + '.pt', weights_only=True)
        net = _finetuner(root, 'c')
        for name in sd['names']:
            if name.startswith('conv'):
                assert torch.equal(net.variable(name).cpu(), sd[name]), name
        assert [n for n in net.variables() if n.startswith('conv')] == [n for n in sd['names'] if n.startswith('conv')]
        assert tuple(net.variable('newfc1/weights').shape) == (_laplacians('c')[1].shape[0] * s['F'][-1], HEAD[0])
        assert tuple(net.variable('newlogits/bias').shape) == (HEAD[-1],)
    with pytest.raises(ValueError, match='K'):
        models_gcn.finetuning_cgcnn({'device': DEV}, root, _laplacians('c'), s['F'], [3, 3, 3], s['p'], HEAD, channel=2,
                                    dir_name='pre', verbose=False)


@pytest.mark.parametrize('shape', ['a', 'b', 'c'])
def test_logits_vs_float64(home, shape):
    root, pre = _pretrained(home, shape)
    net = _finetuner(root, shape)
    net._shape = shape
    if shape == 'b':
        assert net._orders[-1] is not None, 'graph (b) must run in a relabelled vertex order'
    x, y, xs, _ = _batch(net, shape)
    with torch.no_grad():
        got = net._inference_storage(xs, 1).cpu().numpy()
    ref, _, _ = _reference(net, _vars(net), x, y)
    err = _rel(got, ref)
    record_measured('finetune_logits', shape=shape, rel_err=err)
    assert err <= 1e-5, err


CASES = [('a', False, None), ('a', True, None), ('b', True, ['conv2']), ('c', True, ['conv2'])]


@pytest.mark.parametrize('shape,tuning,layers', CASES)
def test_one_step_gradients_and_frozen_trunk(home, shape, tuning, layers):
    root, pre = _pretrained(home, shape)
    net = _finetuner(root, shape, flag_tuning=tuning, train_layers=layers)
    net._shape = shape
    net.enable_step_graph(False)
    x, y, xs, yd = _batch(net, shape)
    P0 = _vars(net)
    frozen = [n for n in net.variables() if n not in net._trainable]
    if tuning and layers is None:
        assert net.train_layers == ['conv4', 'conv5', 'conv6']
    before = {n: net.variable(n).detach().clone() for n in frozen}
    net._grad[net._n_train:].fill_(float('nan'))         # frozen gradient slots: never written
    _lib.dispatch_log = []
    try:
        net.train_step(xs, yd)
        torch.cuda.synchronize()
        log = list(_lib.dispatch_log)
    finally:
        _lib.dispatch_log = None
    _, loss_ref, G = _reference(net, P0, x, y)
    for name in net._trainable:
        got = net.gradient(name).detach().cpu().numpy().astype(np.float64)
        err = _rel(got, G[name])
        record_measured('finetune_grad', shape=shape, tuning=tuning, var=name, rel_err=err)
        assert err <= 2e-4, (name, err)
    assert sorted(G) == sorted(net._trainable)
    assert bool(torch.isnan(net._grad[net._n_train:]).all())
    # the step's parameters: Nadam (t = 1) with the L2 term on the new* variables, against float64
    lr_t = 0.001 * np.sqrt(1 - 0.999) / (1 - 0.9)
    for name in net._trainable:
        g = G[name] + (net.regularization * P0[name] if name in net.regularizers else 0)
        m, v = (1 - B1) * g, (1 - B2) * g * g
        want = P0[name] - ((1 - B1) * g + B1 * m) * lr_t / (np.sqrt(v) + 1e-8)
        got = net.variable(name).detach().cpu().numpy().astype(np.float64)
        well = np.abs(g) > 1e-5                          # elsewhere the update is ill-conditioned in fp32 (eps = 1e-8)
        assert np.abs(got - want)[well].max(initial=0) <= 2e-3 * lr_t, name
        assert np.abs(got - P0[name]).max() <= 1.01 * 0.19 / np.sqrt(0.001) * lr_t, name
    # the loss the bookkeeping reported: cross-entropy + reg * sum l2_loss of the new* variables before the update
    assert abs(float(net._loss_ema) - 0.1 * loss_ref) <= 1e-5 * abs(loss_ref)
    for _ in range(4):
        net.train_step(xs, yd)
    torch.cuda.synchronize()
    for n in frozen:
        assert torch.equal(net.variable(n), before[n]), n
    assert bool(torch.isnan(net._grad[net._n_train:]).all())
    # every step names the Nadam kernel and the library's FC kernels for newfc1
    by = lambda what: [d for w, d in log if w == what]
    assert by('nadam_step_sq_all') == ['nadam_sq_kernel<all>']
    assert len(by('fc_fwd')) == len(HEAD) and all('fc_fwd_kernel' in d for d in by('fc_fwd'))       # no vendor GEMM
    assert len(by('fc_bwd')) == len(HEAD) and all('fc_bwd_w_kernel' in d for d in by('fc_bwd'))
    assert by('planes_to_rows') == ['planes_rows_kernel<to_rows>']
    if tuning:
        assert 'planes_rows_kernel<to_planes>' in [d for w, d in log]
    else:
        assert not any(w.startswith(('fused_layer_bwd', 'contract_bwd', 'recurrence_bwd')) for w, _ in log)


def test_nadam_kernel_partials_and_bookkeeping():
    """Three steps against float64 Nadam (lr_t by value, from device memory, by value), the partial sums of squares of the
    regularised prefix and the loss average chebgcn_loss_bookkeeping makes of them."""
    rs = np.random.RandomState(1)
    n, r, reg = 300007, 123457, 3e-3
    p = rs.randn(n).astype(np.float32)
    dp, dm, dv, dg = torch.as_tensor(p, device=DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    sq = torch.zeros(4096, device=DEV)
    ema = torch.zeros((), device=DEV)
    P, Mo, V, E = p.astype(np.float64), np.zeros(n), np.zeros(n), 0.0
    for t in (1, 2, 3):
        g = (rs.randn(n) * 10.0 ** rs.uniform(-3, 0, n)).astype(np.float32)
        lr_t = 0.001 * np.sqrt(1 - 0.999 ** t) / (1 - 0.9 ** t)
        lr_arg = float(lr_t) if t != 2 else torch.tensor([lr_t], dtype=torch.float32, device=DEV)
        ce = torch.tensor(0.7 + t, device=DEV)
        dg.copy_(torch.as_tensor(g, device=DEV))
        nparts = ops.nadam_step_sq_all(dp, dg, dm, dv, r, lr_arg, sq, 0.9, 0.999, 1e-8, 1.0, reg)
        assert _lib.last_dispatch() == 'nadam_sq_kernel<all>'
        la = ops.loss_bookkeeping(ce, sq, nparts, 0.5 * reg, ema, 1.0)
        G = g.astype(np.float64)
        G[:r] += reg * P[:r]
        sq_ref = np.sum(P[:r] ** 2)
        Mo += (1 - B1) * (G - Mo)
        V += (1 - B2) * (G * G - V)
        P = P - ((1 - B1) * G + B1 * Mo) * np.float32(lr_t) / (np.sqrt(V) + 1e-8)
        E += 0.1 * ((0.7 + t) + 0.5 * reg * sq_ref - E)
        assert abs(float(sq[:nparts].double().sum()) - sq_ref) <= 1e-5 * sq_ref
        assert abs(float(la) - E) <= 1e-5 * abs(E)
        for got, ref, what in ((dm, Mo, 'm'), (dv, V, 'v'), (dp, P, 'p')):
            got = got.cpu().numpy().astype(np.float64)
            if what == 'p':                     # fp32 storage of p: its rounding, plus 1e-3 of a step
                assert np.all(np.abs(got - ref) <= 1e-6 * np.abs(ref) + 1e-3 * lr_t), (t, what)
            else:
                assert _rel(got, ref) <= 2e-6, (t, what)


def test_momentum_zero_is_gradient_descent(home):
    root, _ = _pretrained(home, 'c')
    net = _finetuner(root, 'c', momentum=0, learning_rate=0.05, flag_tuning=True, train_layers=['conv3'])
    x, y, xs, yd = _batch(net, 'c')
    frozen = {n: net.variable(n).detach().clone() for n in net.variables() if n not in net._trainable}
    for step in range(3):
        P0 = _vars(net)
        net.train_step(xs, yd)
        for name in net._trainable:
            g = net.gradient(name).detach().cpu().numpy().astype(np.float64)
            g = g + (net.regularization * P0[name] if name in net.regularizers else 0)
            want = P0[name] - 0.05 * g
            got = net.variable(name).detach().cpu().numpy().astype(np.float64)
            assert np.abs(got - want).max() <= 1e-6 * max(np.abs(want).max(), 1.0), (step, name)
    for n, v in frozen.items():
        assert torch.equal(net.variable(n), v)


@pytest.mark.parametrize('tuning', [False, True])
def test_captured_step_equals_eager(home, tuning):
    root, _ = _pretrained(home, 'a')
    nets = [_finetuner(root, 'a', flag_tuning=tuning) for _ in range(2)]
    nets[1].load_state_dict(nets[0].state_dict())
    nets[0].enable_step_graph(True)
    nets[1].enable_step_graph(False)
    _, _, xs, yd = _batch(nets[0], 'a')
    for step in range(6):
        la = [float(n.train_step(xs, yd)[1]) for n in nets]
        assert la[0] == la[1], (step, la)
    assert nets[0]._sg is not None and nets[1]._sg is None
    for name in nets[0].variables():
        assert torch.equal(nets[0].variable(name), nets[1].variable(name)), name


def test_fit_twice_and_predict_from_own_checkpoint(home, monkeypatch):
    root, pre = _pretrained(home / 'pre_home', 'c')
    monkeypatch.setenv('CHEBGCN_HOME', str(home / 'ft_home'))
    rs = np.random.RandomState(9)
    M0 = _laplacians('c')[0].shape[0]
    xtr, ytr = rs.randn(40, M0, 2).astype(np.float32), rs.randint(0, HEAD[-1], 40)
    xte, yte = rs.randn(13, M0, 2).astype(np.float32), rs.randint(0, HEAD[-1], 13)
    net = _finetuner(root, 'c', num_epochs=2, eval_frequency=3, dir_name='pre')
    trunk = {n: net.variable(n).detach().clone() for n in net.variables() if n.startswith('conv')}
    runs = []
    for _ in range(2):
        np.random.seed(0)
        torch.manual_seed(0)
        acc, losses, _ = net.fit(xtr, ytr, xte, yte)
        assert net.fit_captured
        runs.append((acc, losses, _vars(net)))
    assert runs[0][0] == runs[1][0] and runs[0][1] == runs[1][1]
    for name in net.variables():
        assert np.array_equal(runs[0][2][name], runs[1][2][name]), name
    for n, v in trunk.items():
        assert torch.equal(net.variable(n), v), n
    # the fine-tuned checkpoint alone: the pretrained directory is gone
    shutil.rmtree(str(home / 'pre_home'))
    ckp = str(home / 'ft_home') + '/checkpoints/pre'
    logits, labels, loss, _ = models_gcn.model_perf().predict(ckp, xte, yte, batch_size=B)
    lines = [l.rstrip('\n').split('"')[1] for l in open(ckp + '/model/checkpoint')]
    net.load_state_dict(torch.load(ckp + '/model/' + lines[1] + '.pt', weights_only=True))
    want = []
    staged = net.stage(xte)
    for begin in range(0, 13, B):
        idx = torch.arange(begin, min(begin + B, 13), dtype=torch.int32, device=DEV)
        x = net._gather(staged, idx)
        pad = ops.plane_empty(B, 2, M0, DEV, zero=True)
        pad[:len(idx)] = x.planes
        with torch.no_grad():
            want.append(net._inference_storage(net.as_internal(pad), 1).cpu().numpy())
    want = np.stack(want).flatten()[:13]
    assert np.array_equal(logits, want)
    assert np.array_equal(labels, net.predict(xte))
