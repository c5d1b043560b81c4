"""``predict_mc`` end to end on the MI355X (``-m gpu``): small nets of tests/test_gpu_saliency.py -- 'a3' (on-chip trunk), 'b'
(relabelled, N = 1200), 'c_max' (pooling), 'fourier', and 'a3_deep', a copy of 'a3' with M = [24, 12, 5] so that a per-sample
dropout site exists -- against ``uncertainty.mc_host`` on the float64 ``RefNet`` trunk features; n = 10 windows, S = 5 samples.

Bounds.  Sampled logits: REL = 1e-5 of the window's scale (max |reference logit| over its samples), the bound every forward of
this suite is held to.  Measures: the kernel test's bounds, 1e-5 absolute for the mean probabilities and 1e-5 max(1, log C) for
the three entropies -- against the float64 reference (``mc_host``), between batch sizes, and between ``decode_series(mc=)`` on
either path and ``predict_mc`` on the windows cut by hand; nothing is added for the logits' own error.  ``_check_measures``
prints each error as a share of its bound and ``record_measured`` keeps it (measured on an MI355X: sampled logits within 4e-7
of the scale; the largest error of any measure in any of the comparisons 0.024 of its bound).  Votes and labels are compared exactly against the
float64 reduction of the GPU's own logits, and against the reference wherever no sample's top-2 logit gap is within 1e-4 of
the scale."""
import numpy as np
import pytest
import torch

from conftest import record_measured
from gcn_fmri_decoding_amd import _lib, models_gcn, ops, uncertainty
import test_gpu_saliency as sal
from test_decode_host import host_windows
from test_gpu_saliency import DEV, REL, _same, _state
from test_saliency_host import RefNet

pytestmark = pytest.mark.gpu
N, S, KEEP, SEED = 10, 5, 0.5, 11
NAMES = ['a3', 'b', 'c_max', 'fourier', 'a3_deep']


def _spec(name):
    base = 'a3' if name == 'a3_deep' else name
    s = dict(sal.NETS[base])
    if name == 'a3_deep':
        s['M'] = [24, 12, 5]
    return base, s


def _model(name, seed=0, batch_size=4, dropout=KEEP, **kw):
    base, s = _spec(name)
    torch.manual_seed(seed)
    net = models_gcn.cgcnn({'device': DEV}, sal._laplacians(base), s['F'], s['K'], s['p'], s['M'], channel=s['channel'],
                           brelu=s.get('brelu', 'b1relu'), pool=s.get('pool', 'mpool1'), filter=s.get('filter', 'chebyshev5'),
                           batch_size=batch_size, dropout=dropout, verbose=False, **kw)
    net.contraction = 'f32'
    # a head that decides something: weights of unit gain, biases that are not all equal
    rs = np.random.RandomState(5)
    for v in net.variables():
        if v.startswith(('fc', 'logits')):
            shape = tuple(net.variable(v).shape)
            std = 0.5 if v.endswith('bias') else 2.0 / np.sqrt(shape[0])
            net.set_variable(v, (std * rs.randn(*shape)).astype(np.float32))
    return net


def _data(name, seed=1, n=N):
    return sal._data(_spec(name)[0], seed, n)


def _host(name, net, x, windows=None, samples=S, seed=SEED, keep=KEEP):
    """``mc_host`` on the float64 trunk features of ``RefNet`` (a head without layers returns the feature mean)."""
    base, s = _spec(name)
    trunk = RefNet(sal._laplacians(base), s['F'], s['K'], s['p'], [], s.get('filter', 'chebyshev5'), s.get('brelu', 'b1relu'),
                   s.get('pool', 'mpool1'))
    P = {n: net.variable(n).detach().cpu().numpy().astype(np.float64) for n in net.variables()}
    with torch.no_grad():
        feats = trunk.logits({k: torch.as_tensor(v) for k, v in P.items()}, torch.as_tensor(x.astype(np.float64))).numpy()
    return uncertainty.mc_host(feats, P, np.arange(len(x)) if windows is None else windows, samples, seed, keep)


def _scale(ref_logits):
    return np.maximum(np.abs(ref_logits).max(axis=(0, 2)), 1e-30)                     # per window


def _check_measures(what, got, want, C):
    """The measures of ``got`` against ``want`` within the kernel test's bounds; returns each largest error over its bound."""
    pb, hb = 1e-5, 1e-5 * max(1.0, np.log(C))
    errs = {}
    e = np.abs(got['probabilities'].astype(np.float64) - want['probabilities']).max(axis=1)
    errs['probabilities'] = float((e / pb).max())
    for k in ('entropy', 'expected_entropy', 'mutual_information'):
        errs[k] = float((np.abs(got[k].astype(np.float64) - want[k]) / hb).max())
    print(what, {k: '%.3f of the bound' % v for k, v in errs.items()})
    assert all(v <= 1 for v in errs.values()), (what, errs)
    return errs


@pytest.mark.parametrize('name', NAMES)
def test_predict_mc_against_float64(name):
    net = _model(name)
    if name == 'b':
        assert net._relabelled
    x = _data(name)
    C = int(net.M[-1])
    want = _host(name, net, x)
    # an entry point without arms (perm_data, feature_mean) notes no dispatch: in the log it repeats the kernel the process
    # launched last, whichever test that was.  One pass outside the log makes that kernel predict_mc's own.
    net.predict_mc(x, samples=S, seed=SEED)
    saved, _lib.dispatch_log = _lib.dispatch_log, []
    try:
        got = net.predict_mc(x, samples=S, seed=SEED, return_samples=True)
        log = [k for _, k in _lib.dispatch_log]
    finally:
        _lib.dispatch_log = saved
    assert isinstance(got, uncertainty.MCResult) and got.entropy is got['entropy']
    assert got['logits'].shape == (S, N, C) and got['logits'].dtype == np.float32
    assert got['probabilities'].shape == (N, C) and got['votes'].shape == (N, C) and got['votes'].dtype == np.int32
    assert got['labels'].dtype == np.int64 and all(got[k].shape == (N,) for k in ('labels', 'entropy', 'expected_entropy',
                                                                                   'mutual_information', 'agreement'))
    # the kernels: fc1 once per batch, the shared site, a per-sample site where the head has one, the reduction
    assert 'fc_fwd_dropout_kernel<shared>' in log and 'mc_reduce_kernel' in log
    assert ('fc_fwd_dropout_kernel<per_sample>' in log) == (name == 'a3_deep')
    assert not [k for k in log if 'bwd' in k or 'adam' in k or 'xent' in k], log
    scale = _scale(want['logits'])
    err = np.abs(got['logits'].astype(np.float64) - want['logits']).max(axis=(0, 2)) / scale
    print('%s: sampled logits, rel err per window %s' % (name, err))
    assert err.max() <= REL, (name, err)
    errs = _check_measures(name, got, want, C)
    own = uncertainty.mc_measures(got['logits'])
    assert np.array_equal(got['votes'], own['votes']) and (got['votes'].sum(axis=1) == S).all()
    assert np.array_equal(got['agreement'], (got['votes'][np.arange(N), got['labels']] / np.float32(S)).astype(np.float32))
    top = np.sort(want['logits'], axis=2)
    clear = ((top[:, :, -1] - top[:, :, -2]).min(axis=0) > 1e-4 * scale)
    assert clear.sum() >= N // 2
    assert np.array_equal(got['votes'][clear], want['votes'][clear])
    ptop = np.sort(want['probabilities'], axis=1)
    decided = clear & (ptop[:, -1] - ptop[:, -2] > 1e-3)
    assert np.array_equal(got['labels'][decided], want['labels'][decided])
    # dropout does something: the samples differ, and some window is less than unanimous or has mutual information
    assert np.abs(got['logits'][0] - got['logits'][1]).max() > 1e-3 * scale.max()
    assert (got['mutual_information'] > 0).any()
    record_measured('predict_mc_vs_float64', net=name, logits_rel_err=float(err.max()), bound=REL, **errs)


@pytest.mark.parametrize('name', ['a3', 'a3_deep'])
def test_batch_size_seed_and_reruns(name):
    net = _model(name)
    x = _data(name)
    C = int(net.M[-1])
    a = net.predict_mc(x, samples=S, seed=SEED, batch_size=3, return_samples=True)
    b = net.predict_mc(x, samples=S, seed=SEED, batch_size=7, return_samples=True)
    scale = _scale(a['logits'].astype(np.float64))
    err = np.abs(a['logits'].astype(np.float64) - b['logits']).max(axis=(0, 2)) / scale
    assert err.max() <= REL, err                       # (a mask tied to the batch position would differ at O(1))
    errs = _check_measures(name + ' batch 3 against 7', a, {k: v.astype(np.float64) for k, v in b.items()}, C)
    record_measured('predict_mc_batch_3_against_7', net=name, logits_rel_err=float(err.max()), **errs)
    again = net.predict_mc(x, samples=S, seed=SEED, batch_size=3, return_samples=True)
    for k in a:
        assert np.array_equal(a[k].view(np.uint8), again[k].view(np.uint8)), k + ': the same call twice differs'
    other = net.predict_mc(x, samples=S, seed=SEED + 1, batch_size=3, return_samples=True)
    assert np.abs(other['logits'] - a['logits']).max() > 1e-3 * scale.max()
    # more samples: the first S are the same samples; another keep draws other masks
    more = net.predict_mc(x, samples=S + 3, seed=SEED, batch_size=3, return_samples=True)
    assert np.array_equal(more['logits'][:S], a['logits'])
    k8 = net.predict_mc(x, samples=S, seed=SEED, keep=0.8, batch_size=3, return_samples=True)
    want = _host(name, net, x, keep=0.8)
    assert (np.abs(k8['logits'].astype(np.float64) - want['logits']).max(axis=(0, 2)) / _scale(want['logits'])).max() <= REL
    # a subset of the windows, renumbered by the caller's data: window w of x[3:] is window w of that call
    sub = net.predict_mc(x[3:], samples=S, seed=SEED, return_samples=True)
    want = _host(name, net, x[3:])
    assert (np.abs(sub['logits'].astype(np.float64) - want['logits']).max(axis=(0, 2)) / _scale(want['logits'])).max() <= REL


def test_model_state_rng_and_vendor_gemm(monkeypatch):
    name = 'a3_deep'
    x = _data(name, n=4)
    labels = torch.as_tensor(np.arange(4) % 5, dtype=torch.int64, device=DEV)
    a = _model(name, seed=7, dropout=1)               # (trained without dropout: the captured step draws nothing)
    a.enable_step_graph(True)
    xs = a._gather(a.stage(x), torch.arange(4, dtype=torch.int32, device=DEV))
    for _ in range(3):
        a.train_step(xs, labels)                      # two eager steps, then the captured one
    assert a._sg is not None
    torch.cuda.synchronize()
    before, sg, grad_view = _state(a), a._sg, a.gradient('conv1/weights').clone()
    rng_dev, rng_cpu = torch.cuda.get_rng_state(DEV), torch.get_rng_state()
    xm = _data(name)
    pred = a.predict(xm)
    ser = xm[:, :, 0].copy()                          # [T = 10, M]: 8 windows of 3 time points
    dec = {share: a.decode_series(ser, share=share) for share in (False, True)}

    def no_gemm(*args, **kw):
        raise AssertionError('predict_mc called a vendor GEMM')
    timers = ops.KernelTimers()
    with monkeypatch.context() as m:
        m.setattr(torch, 'addmm', no_gemm)
        m.setattr(torch, 'matmul', no_gemm)
        m.setattr(torch, 'mm', no_gemm)
        ops.timers = timers
        saved, _lib.dispatch_log = _lib.dispatch_log, []
        try:
            a.training_mode = True
            before[-1] = True
            a.predict_mc(xm, samples=S, seed=SEED, keep=KEEP)
            a.predict_mc(xm, samples=3, seed=1, keep=0.9, batch_size=7, return_samples=True)
            a.decode_series(ser, share=False, mc=dict(samples=2, keep=KEEP))
            a.decode_series(ser, share=True, mc=dict(samples=2, keep=KEEP))
            log = list(_lib.dispatch_log)
        finally:
            ops.timers, _lib.dispatch_log = None, saved
    torch.cuda.synchronize()
    assert _same(_state(a), before)
    assert a._sg is sg and a._step_graph_on and torch.equal(a.gradient('conv1/weights'), grad_view)
    assert a._mc is None and a._windows is None and a._pass is None
    assert torch.equal(torch.cuda.get_rng_state(DEV), rng_dev) and torch.equal(torch.get_rng_state(), rng_cpu)
    assert not [w for w, k in log if 'bwd' in w or 'bwd' in k or 'adam' in w or 'adam' in k or 'xent' in k], log
    assert {'fc_fwd_dropout', 'mc_reduce', 'fc_fwd'} <= set(timers.records) and not [k for k in timers.records if 'bwd' in k or 'adam' in k]
    # S samples cost one trunk pass: per batch one fc1 launch and one reduction, (sites) dropout launches
    nb = 3 + 2 + 2 + 2                                                   # batches of the four calls (10 / 4, 10 / 7, 8 / 4, 8 / 4 windows)
    assert len(timers.records['mc_reduce']) == nb and len(timers.records['fc_fwd']) == nb
    assert len(timers.records['fc_fwd_dropout']) == 2 * nb
    # what predict and decode_series returned before the first Monte-Carlo call, they return after it: bit for bit
    a.training_mode = False
    assert np.array_equal(a.predict(xm), pred)
    for share in (False, True):                                          # (both paths thread the Monte-Carlo state through)
        assert np.array_equal(a.decode_series(ser, share=share), dec[share]), share


@pytest.mark.parametrize('name', ['a3', 'b'])
def test_decode_series_mc_equals_predict_mc_on_the_windows(name):
    net = _model(name)
    base, s = _spec(name)
    C = s['channel']
    rs = np.random.RandomState(3)
    runs = [rs.randn(T, sal._laplacians(base)[0].shape[0]).astype(np.float32) for T in (C + 6, C + 2)]
    starts = [np.arange(0, r.shape[0] - C + 1) for r in runs]
    x = np.concatenate([host_windows(r, st, C) for r, st in zip(runs, starts)])
    want = net.predict_mc(x, samples=S, seed=SEED, batch_size=4, return_samples=True)
    w64 = {k: v.astype(np.float64) for k, v in want.items()}
    n0 = len(starts[0])
    for share in (True, False):
        outs = net.decode_series(runs, share=share, batch_size=3, mc=dict(samples=S, seed=SEED))
        assert net.last_decode_path == ('shared' if share else 'materialised')
        assert isinstance(outs, list) and [len(o['labels']) for o in outs] == [len(st) for st in starts]
        for o, sl in zip(outs, (slice(0, n0), slice(n0, None))):       # window numbers run on across the runs
            assert isinstance(o, uncertainty.MCResult) and 'logits' not in o
            errs = _check_measures('%s share=%s' % (name, share), o, {k: v[sl] for k, v in w64.items() if k != 'logits'},
                                   int(net.M[-1]))
            record_measured('decode_series_mc_vs_predict_mc', net=name, share=int(share), **errs)
            assert np.array_equal(o['votes'].sum(axis=1), np.full(len(o['labels']), S))
    one = net.decode_series(runs[0], share=False, mc=dict(samples=S, seed=SEED))
    assert isinstance(one, uncertainty.MCResult)
    _check_measures(name + ' one run', one, {k: v[:n0] for k, v in w64.items() if k != 'logits'}, int(net.M[-1]))
    if name == 'a3':
        with pytest.raises(ValueError, match='samples'):
            net.decode_series(runs, mc=dict(samples=0))


def test_model_perf_predict_mc_from_fit_checkpoint(tmp_path, monkeypatch):
    name = 'a3'
    monkeypatch.setenv('CHEBGCN_HOME', str(tmp_path))
    xtr = _data(name, seed=11, n=16)
    ytr = np.arange(16) % 5
    net = _model(name, dropout=1, num_epochs=2, eval_frequency=2, dir_name='mc')
    net.fit(xtr, ytr, xtr[:8], ytr[:8])
    root = str(tmp_path) + '/checkpoints/mc'
    x = _data(name)
    got = models_gcn.model_perf().predict_mc(root, x, batch_size=4, samples=S, seed=SEED, keep=0.5)
    live = models_gcn.model_perf._restore(root, 4, model=net)
    want = live.predict_mc(x, samples=S, seed=SEED, keep=0.5)
    assert sorted(got) == sorted(want) == sorted(uncertainty.MEASURES)
    for k in want:
        assert np.array_equal(got[k], want[k]), k


def test_refusals_on_the_device(tmp_path, monkeypatch):
    name = 'c_max'
    base, s = _spec(name)
    monkeypatch.setenv('CHEBGCN_HOME', str(tmp_path))
    pre = _model(name, dir_name='pre')
    pre._save_best(50.0, 7, [])
    ft = models_gcn.finetuning_cgcnn({'device': DEV}, str(tmp_path) + '/checkpoints/', sal._laplacians(base), s['F'], s['K'],
                                     s['p'], [12, 5], channel=s['channel'], dir_name='pre', batch_size=4, verbose=False,
                                     brelu=s['brelu'], pool=s['pool'])
    x = _data(name)
    flat = models_gcn.cgcnn({'device': DEV}, sal._laplacians(base), s['F'], s['K'], s['p'], [5], channel=s['channel'],
                            brelu=s['brelu'], pool=s['pool'], batch_size=4, dropout=0.5, verbose=False)
    full = _model(name, dropout=1)
    torch.cuda.synchronize()
    saved, _lib.dispatch_log = _lib.dispatch_log, []
    try:
        with pytest.raises(NotImplementedError, match='finetuning_cgcnn'):
            ft.predict_mc(x, keep=0.5)
        with pytest.raises(NotImplementedError, match='finetuning_cgcnn'):
            ft.decode_series(x[:, :, 0].copy(), mc=dict(keep=0.5))
        with pytest.raises(ValueError, match='hidden FC layer'):
            flat.predict_mc(x)
        with pytest.raises(ValueError, match='dropout'):
            full.predict_mc(x)
        assert _lib.dispatch_log == [], 'a refused call launched %s' % _lib.dispatch_log
    finally:
        _lib.dispatch_log = saved
