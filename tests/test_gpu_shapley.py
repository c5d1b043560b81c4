"""Shapley maps (base_model.shapley / shapley_maps, model_perf.shapley_maps) on the MI355X, on two of the networks of
tests/test_gpu_occlusion.py -- the atlas shape (six fused layers) and a relabelled graph of more than 1024 vertices pooled
through index maps -- and on finetuning_cgcnn with a frozen and with a tuned trunk, at batch sizes that split a window's rows
across passes and that hold several windows.

* Efficiency: a window's attributions sum to s(x) - s(baseline window), both scored from the logits ``predict`` forms.
* Against ``shapley_host`` (tests/test_shapley_host.py) driven by the float64 restatement of the network, with the call's own
  permutation table.
* At G = 2, P = 2, antithetic, the two permutations are all there are: the exact Shapley values, from ``occlusion``'s drops.

The bound is the one tests/test_gpu_occlusion.py holds a drop to against its restatement: REL of the window's scale (max |z|
of its own logits).  A Shapley value is the mean of P differences of two scores, each score as far from float64 as
occlusion's, so the mean is held to the same figure.  That file's margin rule applies: no window is exempt on account of a
ReLU or max-pool decision (the score is continuous in them; the margins are recorded); a window whose two largest float64
logits lie within TIE of each other may be given the other class under 'predicted' and is then not held to the bound.  The
restatement is scored for the class the GPU chose.  At least three of the ten windows must be held to the bound."""
import numpy as np
import pytest
import torch

from conftest import record_measured
from gcn_fmri_decoding_amd import _lib, attribution, models_gcn, ops
from test_gpu_occlusion import TIE, FineRefNet, _finetuner, _reference
from test_gpu_saliency import BS, NETS, REL, S, _data, _model
from test_shapley_host import shapley_host

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)


def _groups(M, G=6):
    """G groups and vertices outside the game (-1, about one in G + 1); every id occurs."""
    g = np.random.RandomState(6).randint(-1, G, M)
    g[:G] = np.arange(G)
    return g


def _baseline(x, seed=5):
    return 0.5 * np.random.RandomState(seed).randn(*x.shape[1:]).astype(np.float32)


def _scores(z, t, score):
    """s_c of logits z [S, C] for classes t, in float64."""
    z = np.asarray(z, np.float64)
    if score == 'logprob':
        m = z.max(axis=1, keepdims=True)
        z = z - (m + np.log(np.exp(z - m).sum(axis=1, keepdims=True)))
    return z[np.arange(len(z)), t]


def _predict_logits(net, x):
    """The logits ``predict`` forms for ``x``: batches of the model's batch size, the last one zero-padded."""
    data = net.stage(x)
    out = []
    was = net.training_mode
    net.training_mode = False
    try:
        for begin in range(0, len(x), net.batch_size):
            idx = torch.arange(begin, min(begin + net.batch_size, len(x)), dtype=torch.int32, device=DEV)
            with torch.no_grad():
                z = net._inference_storage(net.as_internal(net._gather_padded(data, idx, net.batch_size)), 1)
            out.append(z[:idx.numel()].cpu().numpy())
    finally:
        net.training_mode = was
    return np.concatenate(out)


def _total(net, x, groups, baseline, t, score):
    """s(x_w) - s(baseline window) per window from predict's logits, and the windows' scale max |z|.  The baseline window
    keeps the window's own values on the vertices of group -1."""
    g = np.arange(x.shape[1]) if groups is None else np.asarray(groups)
    x0 = np.zeros(x.shape[1:], np.float32) if baseline is None else baseline
    empty = np.where((g < 0)[None, :, None], x, x0[None]).astype(np.float32)
    z, z0 = _predict_logits(net, x), _predict_logits(net, empty)
    return _scores(z, t, score) - _scores(z0, t, score), np.abs(z).max(axis=1)


def _check_efficiency(tag, net, x, phi, t, groups, baseline, score):
    want, scale = _total(net, x, groups, baseline, t, score)
    err = np.abs(phi.astype(np.float64).sum(axis=1) - want) / scale
    record_measured('shapley_efficiency', case=tag, score=score, rel_err=float(err.max()), bound=REL,
                    total_scale=float((np.abs(want) / scale).max()))
    assert np.abs(want).max() > 0, tag
    assert err.max() <= REL, '%s %s: the row sums miss s(x) - s(baseline) by %.3e (window %d)' % (
        tag, score, err.max(), int(np.argmax(err)))


def _check_float64(tag, ref, P, x, phi, t, target, score, groups, baseline, perms):
    """phi / t of one call against shapley_host over the float64 network, scored for the GPU's classes."""
    xs = x.astype(np.float64)
    ref.margin = None                                   # per call of ref.logits: its rows differ from call to call
    with torch.no_grad():
        z = ref.logits(P, torch.as_tensor(xs)).numpy()
    zs = np.sort(z, axis=1)
    scale = np.abs(z).max(axis=1)
    gap = (zs[:, -1] - zs[:, -2]) / scale
    keep = np.ones(len(x), bool)
    if isinstance(target, str) and target == 'predicted':
        keep = gap > TIE
        assert np.array_equal(t[keep], np.argmax(z, axis=1)[keep]), (tag, t, np.argmax(z, axis=1), gap)
    want, margin = np.empty(phi.shape), np.empty(len(x))
    for w in range(len(x)):
        ref.margin = None

        def f(rows, c=t[w]):
            with torch.no_grad():
                return ref.score(P, torch.as_tensor(rows), np.full(len(rows), c), score).numpy()
        want[w] = shapley_host(f, xs[w:w + 1], groups, baseline, perms)[0]
        margin[w] = ref.margin.min()
    assert phi.dtype == np.float32 and phi.shape == want.shape and t.dtype == np.int64 and t.shape == (len(x),)
    err = np.abs(phi.astype(np.float64) - want).max(axis=1) / scale
    record_measured('shapley_vs_float64', case=tag, score=score, target=target if isinstance(target, str) else 'given',
                    rel_err=float(err[keep].max()), all_windows_err=float(err.max()), bound=REL, windows=int(keep.sum()),
                    min_margin=float(margin.min()), min_tie_gap=float(gap.min()),
                    phi_scale=float((np.abs(want).max(axis=1) / scale).max()))
    assert keep.sum() >= 3, (tag, gap)
    assert np.abs(want).max() > 0, tag
    assert err[keep].max() <= REL, '%s %s: %.3e (window %d)' % (tag, score, err[keep].max(), int(np.argmax(err * keep)))


# (groups, baseline?, score, target, permutations, antithetic, batch size): with G = 6 a window has P * 7 rows -- 28 or 21 --
# so 17 and 9 split a window's rows across passes (and start passes mid-permutation), 64 holds several windows
CASES = [(6, False, 'logit', 'predicted', 4, True, 17), (6, True, 'logprob', 'label', 3, True, 64),
         (3, True, 'logit', 2, 3, False, 9)]


@pytest.mark.parametrize('name', ['a3', 'c_maps'])
def test_shapley_against_float64_and_efficiency(name):
    net = _model(name)
    if name == 'c_maps':
        assert net._relabelled and net._pool_maps[0] is not None
    ref, P = _reference(name, net)
    x = _data(name)
    labels = np.random.RandomState(4).randint(0, NETS[name]['M'][-1], S)
    for G, with_base, score, target, nperm, anti, bs in CASES:
        groups, baseline = _groups(x.shape[1], G), _baseline(x) if with_base else None
        phi, t = net.shapley(x, target, score, groups, baseline, nperm, anti, seed=3, batch_size=bs, labels=labels)
        if target == 'label':
            assert np.array_equal(t, labels)
        perms = attribution.shapley_permutations(G, nperm, anti, 3)
        tag = '%s/G%d/P%d/bs%d' % (name, G, nperm, bs)
        _check_float64(tag, ref, P, x, phi, t, target, score, groups, baseline, perms)
        _check_efficiency(tag, net, x, phi, t, groups, baseline, score)
    assert net._pass is None


@pytest.mark.parametrize('tuning', [False, True])
def test_finetuning_cgcnn_shapley(tmp_path, monkeypatch, tuning):
    ft = _finetuner(tmp_path, monkeypatch, tuning)
    ref, P = _reference('a3', ft, FineRefNet)
    x = _data('a3')
    labels = np.arange(S) % 5
    groups, baseline = _groups(x.shape[1]), _baseline(x)
    for score, target, bs in (('logit', 'predicted', 19), ('logprob', 'label', 50)):
        phi, t = ft.shapley(x, target, score, groups, baseline, permutations=3, seed=1, batch_size=bs, labels=labels)
        perms = attribution.shapley_permutations(6, 3, True, 1)
        tag = 'finetune%d/bs%d' % (tuning, bs)
        _check_float64(tag, ref, P, x, phi, t, target, score, groups, baseline, perms)
        _check_efficiency(tag, ft, x, phi, t, groups, baseline, score)
    maps, counts = ft.shapley_maps(x, labels, groups=groups, permutations=3, batch_size=50)
    assert maps.shape == (5, 6) and np.array_equal(counts, np.bincount(labels, minlength=5))


@pytest.mark.parametrize('name', ['a3', 'c_maps'])
@pytest.mark.parametrize('score', ['logit', 'logprob'])
def test_two_groups_two_antithetic_permutations_are_exact(name, score):
    """phi_g = (drop_g + (s(x) - s(baseline) - drop_other)) / 2 with occlusion's drops on the same groups and baseline."""
    net = _model(name)
    x = _data(name)
    M = x.shape[1]
    groups = (np.arange(M) >= M // 3).astype(np.int64)
    groups[::7] = -1
    baseline = _baseline(x)
    phi, t = net.shapley(x, 'predicted', score, groups, baseline, permutations=2, antithetic=True, seed=9, batch_size=5)
    drop, td = net.occlusion(x, t, score, groups, baseline)
    assert np.array_equal(td, t)
    total, scale = _total(net, x, groups, baseline, t, score)
    d = drop.astype(np.float64)
    want = 0.5 * (d + (total[:, None] - d[:, ::-1]))
    err = np.abs(phi.astype(np.float64) - want).max(axis=1) / scale
    record_measured('shapley_exact_two_groups', net=name, score=score, rel_err=float(err.max()), bound=REL)
    assert np.abs(want).max() > 0
    assert err.max() <= REL, (name, score, err)


def test_vertices_outside_the_game_keep_their_values():
    """The baseline on the vertices of group -1 is never read: changing it there leaves every bit of phi."""
    net = _model('a3')
    x = _data('a3')
    groups, baseline = _groups(x.shape[1]), _baseline(x)
    other = baseline.copy()
    other[groups < 0] += 3.0
    a, ta = net.shapley(x, 1, 'logprob', groups, baseline, permutations=3, batch_size=40)
    b, tb = net.shapley(x, 1, 'logprob', groups, other, permutations=3, batch_size=40)
    assert np.array_equal(a, b) and np.array_equal(ta, tb)
    moved = baseline.copy()
    moved[groups == 0] += 3.0
    c, _ = net.shapley(x, 1, 'logprob', groups, moved, permutations=3, batch_size=40)
    assert not np.array_equal(a, c)


@pytest.mark.parametrize('name', ['a3', 'c_maps'])
def test_predicted_target_is_predicts_class(name):
    net = _model(name)
    x = _data(name)
    _, t = net.shapley(x, groups=_groups(x.shape[1], 3), permutations=1, batch_size=7)
    assert np.array_equal(t, net.predict(x).astype(np.int64))


@pytest.mark.parametrize('name', ['a3', 'c_maps'])
def test_shapley_maps_are_class_means_of_shapley_bit_for_bit(name):
    net = _model(name)
    x = _data(name)
    C = NETS[name]['M'][-1]
    labels = np.array([0, 1, 3, 0, 3, 3, 1, 0, 0, 3])         # classes 2 and 4 have no window
    groups, baseline = _groups(x.shape[1]), _baseline(x)
    kw = dict(score='logprob', groups=groups, baseline=baseline, permutations=3, seed=2, batch_size=30)
    maps, counts = net.shapley_maps(x, labels, **kw)
    phi, t = net.shapley(x, target=labels, **kw)
    assert np.array_equal(t, labels)
    assert maps.dtype == np.float64 and maps.shape == (C, 6)
    assert counts.dtype == np.int64 and np.array_equal(counts, np.bincount(labels, minlength=C))
    want = np.zeros((C, 6))
    for w, k in enumerate(labels):                      # windows in order, in float64
        want[k] += phi[w].astype(np.float64)
    want /= np.maximum(counts, 1)[:, None]
    assert np.array_equal(maps, want)
    assert not maps[2].any() and not maps[4].any()


def test_reruns_bit_identical_seeds_differ_and_table_split(monkeypatch):
    net = _model('a3')
    x = _data('a3')
    groups, baseline = _groups(x.shape[1]), _baseline(x)
    kw = dict(target='predicted', score='logit', groups=groups, baseline=baseline, permutations=4, batch_size=33)
    a, ta = net.shapley(x, seed=0, **kw)
    b, tb = net.shapley(x, seed=0, **kw)
    assert np.array_equal(a, b) and np.array_equal(ta, tb)
    c, tc = net.shapley(x, seed=1, **kw)
    assert np.array_equal(tc, ta) and not np.array_equal(a, c)
    _, scale = _total(net, x, groups, baseline, ta, 'logit')
    err = np.abs(a.astype(np.float64).sum(axis=1) - c.astype(np.float64).sum(axis=1)) / scale
    record_measured('shapley_seed_row_sums', rel_err=float(err.max()), bound=REL)
    assert err.max() <= REL, err
    # A score table bound that holds three windows' tables (4 * 7 floats each): four chunks.  At 14 rows a pass, two passes a
    # permutation pair, every pass holds the same rows at the same places as in the unsplit call: the same bits.
    kw['batch_size'] = 14
    whole, _ = net.shapley(x, seed=0, **kw)
    monkeypatch.setattr(ops, 'SHAPLEY_TABLE_BYTES', 3 * 4 * 28 + 5)
    split, ts = net.shapley(x, seed=0, **kw)
    assert np.array_equal(ts, ta) and np.array_equal(split, whole)


def _boom(*a, **k):
    raise AssertionError('the Shapley pass called the vendor GEMM')


@pytest.mark.parametrize('name', ['a3', 'c_maps'])
def test_pass_launches_no_backward_optimizer_or_gemm(name, monkeypatch):
    net = _model(name)
    x = _data(name)
    monkeypatch.setattr(torch, 'addmm', _boom)
    monkeypatch.setattr(torch, 'matmul', _boom)
    timers = ops.KernelTimers()
    monkeypatch.setattr(ops, 'timers', timers)
    groups = _groups(x.shape[1])
    _lib.dispatch_log = log = []
    try:
        net.shapley(x, score='logprob', groups=groups, permutations=3, batch_size=16)
        kernels = {w: d for w, d in log}
        assert kernels['shapley_rows'] == 'shapley_rows_kernel'
        assert kernels['shapley_score'] == 'shapley_score_kernel<logprob>'
        assert kernels['shapley_reduce'] == 'shapley_reduce_kernel'
        assert kernels['saliency_seed'] == 'saliency_seed_kernel<argmax>'
        del log[:]
        net.shapley_maps(x, np.arange(S) % 5, groups=groups, baseline=np.ones(x.shape[1:], np.float32), permutations=2)
        kernels = {w: d for w, d in log}
        assert kernels['shapley_score'] == 'shapley_score_kernel<logit>'
        assert kernels['occlusion_class_sums'] == 'saliency_class_sum_kernel'
        assert 'saliency_seed' not in kernels
        assert not [d for _, d in log if 'bwd' in d or 'adam' in d], log
    finally:
        _lib.dispatch_log = None
    names = list(timers.records)
    assert 'shapley_rows' in names and 'shapley_score' in names and 'shapley_reduce' in names, names
    bad = [n for n in names if 'bwd' in n or n.startswith('bias_grad') or 'adam' in n]
    assert not bad, bad
    assert net._pass is None


def test_model_perf_shapley_maps_from_fit_checkpoint(tmp_path, monkeypatch):
    name = 'a3'
    monkeypatch.setenv('CHEBGCN_HOME', str(tmp_path))
    xtr = _data(name, seed=11, n=16)
    ytr = np.arange(16) % 5
    net = _model(name, num_epochs=2, eval_frequency=2, dir_name='shap')
    net.fit(xtr, ytr, xtr[:8], ytr[:8])
    root = str(tmp_path) + '/checkpoints/shap'
    x, labels = _data(name), np.arange(S) % 5
    groups = _groups(x.shape[1])
    maps, counts = models_gcn.model_perf().shapley_maps(root, x, labels, batch_size=BS, groups=groups, score='logprob',
                                                        permutations=2)
    live = models_gcn.model_perf._restore(root, BS, model=net)
    want, wcounts = live.shapley_maps(x, labels, groups=groups, score='logprob', permutations=2)
    assert np.array_equal(maps, want) and np.array_equal(counts, wcounts)
