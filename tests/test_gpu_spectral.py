"""Spectral filters on the MI355X (cgcnn filter='fourier' / 'spline', lib_new/models_gcn.py:512-556): every kernel arm by
its name against a float64 restatement, the networks against the reference's logits (tests/golden/inference_{fourier,
spline}_n*.npz) with the fixture's basis injected, one training step's gradients against float64 autograd, three Adam
steps, the spline model's L2 term, the gradients of a Fourier network with average pooling at p = 16 (apool1), a checkpoint
round trip and an eager fit()."""
import numpy as np
import pytest
import torch

from conftest import assert_adam_params_close, csr_from, load_golden, record_measured
from gcn_fmri_decoding_amd import _lib, ops
from gcn_fmri_decoding_amd import graph as graph_mod
from gcn_fmri_decoding_amd import models_gcn
from gcn_fmri_decoding_amd._lib import plane_stride

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
SIZES = [100, 212, 360, 1000, 2000]


def _planes(x, M):
    """[B, F, M] float64 -> [B, F, Mp] fp32 device planes with NaN in the pad (the pad is never read as data)."""
    B, F, _ = x.shape
    out = torch.full((B, F, plane_stride(M)), float('nan'), dtype=torch.float32)
    out[:, :, :M] = torch.as_tensor(x, dtype=torch.float32)
    return out.to(DEV)


def _call(fn, what, expect):
    """Run ``fn`` twice: the two results bit-identical, and the launch reached the kernel ``expect`` names."""
    a = fn()
    assert _lib.last_dispatch() == expect, (_lib.last_dispatch(), expect)
    b = fn()
    torch.cuda.synchronize()
    assert torch.equal(a, b), '%s: two runs differ' % what
    return a.cpu().numpy().astype(np.float64)


def _check(what, got, ref, **tags):
    err = np.abs(got - ref).max() / np.abs(ref).max()
    record_measured(what, rel_err=err, **tags)
    print('%s %s: rel err %.2e' % (what, tags, err))
    assert err <= 1e-5, '%s %s: %.3e' % (what, tags, err)


@pytest.mark.parametrize('M', SIZES)
def test_transform_both_directions(M):
    rs = np.random.RandomState(M)
    U, _ = np.linalg.qr(rs.randn(M, M))            # an orthonormal basis like graph.fourier's
    U32 = U.astype(np.float32).astype(np.float64)
    basis = ops.spectral_basis(U32, DEV)
    B, F = 3, 11                                    # R = 33 planes: one row tile and a partial one
    x = rs.randn(B, F, M)
    x32 = x.astype(np.float32).astype(np.float64)
    xp = _planes(x32, M)
    for transpose, name in ((False, 'spectral_transform_kernel<false>'), (True, 'spectral_transform_kernel<true>')):
        got = _call(lambda: ops.spectral_transform(xp, basis, M, transpose), 'transform', name)
        ref = np.einsum('bfm,jm->bfj', x32, U32) if transpose else np.einsum('bfm,mj->bfj', x32, U32)
        assert np.all(got[:, :, M:] == 0)           # pad of the output: zero
        _check('spectral_transform', got[:, :, :M], ref, M=M, transpose=transpose)


@pytest.mark.parametrize('M', SIZES)
def test_mix_forward_and_gradients(M):
    rs = np.random.RandomState(M + 1)
    B, Fin, Fout = 5, 3, 10                          # none a multiple of the kernels' tiles
    W = rs.randn(M, Fout, Fin).astype(np.float32).astype(np.float64)
    xh = rs.randn(B, Fin, M).astype(np.float32).astype(np.float64)
    dyh = rs.randn(B, Fout, M).astype(np.float32).astype(np.float64)
    Wd = torch.as_tensor(W, dtype=torch.float32).to(DEV)
    xp, dp = _planes(xh, M), _planes(dyh, M)

    got = _call(lambda: ops.spectral_mix(xp, Wd, M), 'mix_fwd', 'spectral_mix_kernel<false>')
    assert np.all(got[:, :, M:] == 0)
    _check('spectral_mix_fwd', got[:, :, :M], np.einsum('mof,bfm->bom', W, xh), M=M)

    got = _call(lambda: ops.spectral_mix(dp, Wd, M, transpose=True), 'mix_bwd_x', 'spectral_mix_kernel<true>')
    assert np.all(got[:, :, M:] == 0)
    _check('spectral_mix_bwd_x', got[:, :, :M], np.einsum('mof,bom->bfm', W, dyh), M=M)

    got = _call(lambda: ops.spectral_mix_bwd_w(dp, xp, M), 'mix_bwd_w', 'spectral_mix_bwd_w_kernel')
    _check('spectral_mix_bwd_w', got, np.einsum('bom,bfm->mof', dyh, xh), M=M)


@pytest.mark.parametrize('M', SIZES)
def test_spline_expand_and_gradient(M):
    rs = np.random.RandomState(M + 2)
    K, C = 7, 15 * 32
    lamb = np.sort(rs.rand(M)).astype(np.float32)
    Bs = np.asarray(models_gcn.bspline_basis(K, lamb), np.float32).astype(np.float64)
    Wk = rs.randn(K, C).astype(np.float32).astype(np.float64)
    dW = rs.randn(M, C).astype(np.float32).astype(np.float64)
    Bd = torch.as_tensor(Bs, dtype=torch.float32).to(DEV)
    got = _call(lambda: ops.spline_expand(Bd, torch.as_tensor(Wk, dtype=torch.float32).to(DEV)), 'expand',
                'spectral_spline_expand_kernel')
    _check('spectral_spline_expand', got, Bs @ Wk, M=M)
    got = _call(lambda: ops.spline_expand(Bd, torch.as_tensor(dW, dtype=torch.float32).to(DEV), transpose=True),
                'expand_bwd', 'spectral_spline_expand_bwd_kernel')
    _check('spectral_spline_expand_bwd', got, Bs.T @ dW, M=M)


def test_spectral_conv_rejects_cpu_tensors():
    x = torch.zeros(1, 2, 32)
    with pytest.raises(_lib.ChebgcnError):
        ops.SpectralConv.apply(x, torch.zeros(10, 3, 2, requires_grad=True), torch.zeros(32, 32), None, 10, 3)


# ---------------------------------------------------------------------------------------------------- networks

NETS = ['inference_fourier_n100', 'inference_fourier_n100_p21', 'inference_spline_n100', 'inference_spline_n100_p21']


def _inject_basis(monkeypatch, z):
    """graph.fourier answers with the fixture's (lamb, U) for each level: the tests pin the kernels, not LAPACK."""
    by_size = {int(z['L%d_shape' % i][0]): (z['lamb%d' % i], z['U%d' % i]) for i in range(int(z['nlevels']))}
    monkeypatch.setattr(graph_mod, 'fourier', lambda L, algo='eigh', k=1: by_size[L.shape[0]])


def _build(z, **kw):
    Ls = [csr_from(z, 'L%d' % i) for i in range(int(z['nlevels']))]
    args = dict(filter=str(z['filter']), brelu=str(z['brelu']), channel=int(z['channel']), batch_size=int(z['x'].shape[0]),
                dropout=1, verbose=False)
    args.update(kw)
    net = models_gcn.cgcnn({'device': DEV}, Ls, z['F'].tolist(), z['K'].tolist(), z['p'].tolist(), z['M'].tolist(), **args)
    for k in z.files:
        if k.startswith('param:'):
            net.set_variable(k[len('param:'):], z[k])
    return net


@pytest.mark.parametrize('name', NETS)
def test_logits_match_reference(monkeypatch, name):
    z = load_golden(name)
    _inject_basis(monkeypatch, z)
    net = _build(z)
    assert not net._fusable() and net.vertex_order == 'reference'
    with torch.no_grad():
        logits = net.inference(torch.as_tensor(z['x']).to(DEV), 1).cpu().numpy()
    ref = z['logits']
    err = np.abs(logits - ref).max() / np.abs(ref).max()
    record_measured('spectral_logits', case=name, rel_err=err)
    assert err < 2e-5, '%s: %.3e' % (name, err)


def _levels(p):
    out, j = [], 0
    for pp in p:
        out.append(j)
        j += int(np.log2(pp)) if pp > 1 else 0
    return out


def _restated_loss(z, params, x, labels, reg, names_reg, pool='mpool1'):
    """The network in float64 torch: filter_in_fourier (:512-528), bias, ReLU, max pooling (``pool='apool1'``: average
    pooling), feature mean, FC head, mean softmax cross-entropy (+ reg * sum of l2_loss over ``names_reg``)."""
    F, K, p, Mfc = z['F'].tolist(), z['K'].tolist(), z['p'].tolist(), z['M'].tolist()
    spline, levels = str(z['filter']) == 'spline', _levels(p)
    h = x
    for i in range(len(F)):
        U = torch.as_tensor(z['U%d' % levels[i]], dtype=torch.float64)
        W = params['conv%d/weights' % (i + 1)]
        N, M, Fin = h.shape
        if spline:
            W = (torch.as_tensor(z['B%d' % i], dtype=torch.float64) @ W).reshape(M, F[i], Fin)
        xh = torch.einsum('jm,njf->nmf', U, h)
        yh = torch.einsum('mof,nmf->nmo', W, xh)
        h = torch.relu(torch.einsum('jm,nmo->njo', U, yh) + params['conv%d/bias' % (i + 1)])
        if p[i] > 1:
            h = h.reshape(N, M // p[i], p[i], F[i])
            h = h.max(dim=2).values if pool == 'mpool1' else h.mean(dim=2)
    h = h.mean(dim=2)
    for i in range(len(Mfc)):
        scope = 'logits' if i == len(Mfc) - 1 else 'fc%d' % (i + 1)
        h = h @ params[scope + '/weights'] + params[scope + '/bias']
        if i < len(Mfc) - 1:
            h = torch.relu(h)
    ce = torch.nn.functional.cross_entropy(h, labels)
    l2 = sum(0.5 * (params[n] ** 2).sum() for n in names_reg) if names_reg else 0.0
    return ce, ce + reg * l2


@pytest.mark.parametrize('name', NETS)
def test_train_step_gradients_and_adam(monkeypatch, name):
    z = load_golden(name)
    _inject_basis(monkeypatch, z)
    reg = 5e-4
    net = _build(z, regularization=reg)
    spline = str(z['filter']) == 'spline'
    assert all(not n.startswith('conv') for n in net.regularizers) if spline else \
        all(('conv%d/weights' % (i + 1)) in net.regularizers for i in range(len(z['F'])))
    B = z['x'].shape[0]
    labels = np.arange(B) % int(z['M'][-1])
    x_dev = torch.as_tensor(z['x']).to(DEV)
    lab_dev = torch.as_tensor(labels).to(DEV)
    params = {n: torch.tensor(z['param:' + n], dtype=torch.float64, requires_grad=True) for n in net.variables()}
    x64 = torch.as_tensor(z['x'], dtype=torch.float64)
    lab64 = torch.as_tensor(labels, dtype=torch.int64)
    m = {n: torch.zeros_like(v) for n, v in params.items()}
    v2 = {n: torch.zeros_like(v) for n, v in params.items()}
    ill = {}
    for step in range(3):
        ce, loss = _restated_loss(z, params, x64, lab64, reg, net.regularizers)
        gce = torch.autograd.grad(ce, list(params.values()), retain_graph=True)
        gall = torch.autograd.grad(loss, list(params.values()))
        _, loss_avg = net.train_step(ops.plane_storage(x_dev), lab_dev)
        if step == 0:
            # the reported loss: 0.1 * (cross-entropy + reg * L2 over the regularised variables only)
            assert abs(float(loss_avg) - 0.1 * float(loss)) <= 2e-5 * abs(0.1 * float(loss))
            for (n, g) in zip(params, gce):
                got = net.gradient(n).detach().cpu().numpy().astype(np.float64)
                ref = g.numpy()
                err = np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-30)
                record_measured('spectral_train_grad', case=name, var=n, rel_err=err)
                assert err <= 5e-5, '%s %s: gradient rel err %.3e' % (name, n, err)
        with torch.no_grad():                         # TF-form Adam, lr 1e-3
            t = step + 1
            lr_t = 1e-3 * np.sqrt(1 - 0.999 ** t) / (1 - 0.9 ** t)
            for (n, p_), g in zip(params.items(), gall):
                m[n].mul_(0.9).add_(0.1 * g)
                v2[n].mul_(0.999).add_(0.001 * g * g)
                p_ -= lr_t * m[n] / (torch.sqrt(v2[n]) + 1e-8)
        for n in params:
            assert_adam_params_close(net.get_var(n), params[n].detach().numpy(), v2[n].numpy(), step, ill, n)


def _ring_laplacian(M):
    """Normalised Laplacian of a ring of M vertices (host CSR, fp32): a level whose basis the test injects."""
    import scipy.sparse as sp
    i = np.arange(M)
    A = sp.coo_matrix((np.ones(2 * M), (np.r_[i, i], np.r_[(i + 1) % M, (i - 1) % M])), shape=(M, M))
    return (sp.identity(M) - 0.5 * A).tocsr().astype(np.float32)


@pytest.mark.parametrize('p', [16])
def test_fourier_apool1_train_step_gradients(monkeypatch, p):
    """cgcnn(filter='fourier', pool='apool1') at a pool the 8-bit ReLU mask does not reach, on a level of 2048 vertices (the
    16-byte-store gradient kernel of the average pooling): one training step's gradients against float64 autograd."""
    M0, Fo, C, B = 2048, 4, 3, 4
    rs = np.random.RandomState(p)
    lamb = np.sort(2 * rs.rand(M0)).astype(np.float32)
    U = np.linalg.qr(rs.randn(M0, M0))[0].astype(np.float32)          # a random orthonormal basis
    Ls = [_ring_laplacian(M0 >> k) for k in range(int(np.log2(p)) + 1)]
    monkeypatch.setattr(graph_mod, 'fourier', lambda L, algo='eigh', k=1: {M0: (lamb, U)}[L.shape[0]])
    reg = 5e-4
    net = models_gcn.cgcnn({'device': DEV}, Ls, [Fo], [3], [p], [C], filter='fourier', pool='apool1', channel=1, batch_size=B,
                           regularization=reg, dropout=1, verbose=False)
    assert not net._fusable() and net.vertex_order == 'reference'
    z = {'F': np.array([Fo]), 'K': np.array([3]), 'p': np.array([p]), 'M': np.array([C]), 'filter': 'fourier', 'U0': U}
    x = rs.randn(B, M0, 1).astype(np.float32)
    labels = np.arange(B) % C
    params = {n: torch.tensor(net.get_var(n), dtype=torch.float64, requires_grad=True) for n in net.variables()}
    ce, loss = _restated_loss(z, params, torch.as_tensor(x, dtype=torch.float64), torch.as_tensor(labels), reg, net.regularizers,
                              pool='apool1')
    gce = torch.autograd.grad(ce, list(params.values()))
    _, loss_avg = net.train_step(ops.plane_storage(torch.as_tensor(x).to(DEV)), torch.as_tensor(labels).to(DEV))
    loss = float(loss.detach())
    assert abs(float(loss_avg) - 0.1 * loss) <= 2e-5 * abs(0.1 * loss)
    for n, g in zip(params, gce):
        got = net.gradient(n).detach().cpu().numpy().astype(np.float64)
        ref = g.numpy()
        err = np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-30)
        record_measured('spectral_apool1_train_grad', p=p, var=n, rel_err=err)
        assert err <= 5e-5, 'apool1 p=%d %s: gradient rel err %.3e' % (p, n, err)


@pytest.mark.parametrize('name', ['inference_fourier_n100_p21', 'inference_spline_n100'])
def test_checkpoint_round_trip(monkeypatch, name):
    z = load_golden(name)
    _inject_basis(monkeypatch, z)
    net = _build(z, regularization=5e-4)
    x = torch.as_tensor(z['x']).to(DEV)
    net.train_step(ops.plane_storage(x), torch.zeros(x.shape[0], dtype=torch.int64, device=DEV))
    with torch.no_grad():
        a = net.inference(x, 1)
    net2 = models_gcn.cgcnn.from_checkpoint(net.state_dict(), {'device': DEV})
    with torch.no_grad():
        b = net2.inference(x, 1)
    assert torch.equal(a, b)


@pytest.mark.parametrize('filt', ['fourier', 'spline'])
def test_fit_runs_eagerly_and_the_loss_falls(monkeypatch, tmp_path, filt):
    z = load_golden('inference_%s_n100' % filt)
    _inject_basis(monkeypatch, z)
    monkeypatch.setenv('CHEBGCN_HOME', str(tmp_path))
    rs = np.random.RandomState(0)
    S, C, M = 40, 5, 100
    labels = np.arange(S) % C
    centres = rs.randn(C, M, 3).astype(np.float32)
    data = (centres[labels] + 0.5 * rs.randn(S, M, 3)).astype(np.float32)
    net = _build(z, num_epochs=2, batch_size=4, eval_frequency=10, regularization=5e-4, dir_name='spectral_fit')
    net.record_fit = True

    def train_ce():
        with torch.no_grad():
            logits = net.inference(torch.as_tensor(data).to(DEV), 1)
            return float(torch.nn.functional.cross_entropy(logits.double(), torch.as_tensor(labels).to(DEV)))
    torch.manual_seed(0)
    net._init_variables()
    before = train_ce()
    torch.manual_seed(0)
    net.fit(data, labels, data[:8], labels[:8])
    after = train_ce()
    assert not net.fit_captured
    assert len(net.fit_log['loss_average']) == 20
    assert np.all(np.isfinite(net.fit_log['loss_average']))
    record_measured('spectral_fit', filter=filt, ce_before=before, ce_after=after)
    assert after < before, (before, after)
