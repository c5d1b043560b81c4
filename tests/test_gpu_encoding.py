"""``ridge_cv`` on the MI355X, end to end: against ``ridge_cv_host`` on the data and with the bound of tests/test_encoding_host.py
(encoding_cases: ``C_BOUND (yy_te + |p| + q) / tss_te`` plus one float32 rounding, ``2^-23 |ref|`` -- the bound also covers the
fma chains of chebgcn_glm_project, which NumPy's ``@`` does not reproduce bit for bit), against the explicit yardstick, and bit
for bit against itself: under any ``batch_runs``, under a permutation of the subjects, with a null 65th feature (the edge of a
64-column call of the statistics), and between tensor and NumPy input.  The fraction of the bound used goes to
``record_measured``.
"""
import numpy as np
import pytest
import torch

import encoding_cases as ec
from conftest import record_measured
from gcn_fmri_decoding_amd import _lib, encoding as en, ridge_cv, ridge_cv_host

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
MAPS = ('score', 'alpha_index', 'weights', 'scores')


def device(duplicate=False, **kw):
    runs, feats = ec.data(duplicate)
    kw.setdefault('groups', ec.GROUPS)
    kw.setdefault('scores', True)
    return ridge_cv(list(runs), list(feats), ec.case_alphas(duplicate), **kw)


def same_bits(a, b, what):
    for name in MAPS:
        x, y = getattr(a, name), getattr(b, name)
        x = x.cpu().numpy() if torch.is_tensor(x) else x
        y = y.cpu().numpy() if torch.is_tensor(y) else y
        assert x.dtype == y.dtype and np.array_equal(x.view(np.uint32), y.view(np.uint32)), '%s: %s differs' % (what, name)


@pytest.fixture(scope='module')
def plain():
    return device()


@pytest.mark.parametrize('duplicate', [False, True])
@pytest.mark.parametrize('kind', ['r2', 'r'])
def test_ridge_cv_against_the_host(duplicate, kind):
    runs, feats = ec.data(duplicate)
    alphas = ec.case_alphas(duplicate)
    got = device(duplicate, score=kind)
    ref = ridge_cv_host(list(runs), list(feats), alphas, groups=ec.GROUPS, score=kind, scores=True)
    assert isinstance(got, en.EncodingResult) and all(isinstance(getattr(got, n), np.ndarray) for n in MAPS)
    assert got.groups == ref.groups and got.folds == ref.folds and np.array_equal(got.alphas, alphas)
    used = 0.0
    for s, (mem, yard) in enumerate(zip(ec.members(), ec.reference(duplicate))):
        scale = yard['scale'].mean(axis=0)
        live = np.isfinite(scale)
        want = ref.scores[s].astype(np.float64)
        assert np.isfinite(got.scores[s]).all() and (got.scores[s][~live] == 0).all()
        err = np.abs(got.scores[s].astype(np.float64) - want)[live]
        bound = ec.C_BOUND * scale[live] + 2.0 ** -23 * np.abs(want[live])
        print('subject %d %s: worst error %.3e, %.3g of its bound' % (s, kind, err.max(), (err / bound).max()))
        assert (err <= bound).all()
        used = max(used, float((err / bound).max()))
        _, _, decided = ec.mean_and_choice(yard[kind])
        assert (~decided).mean() <= 0.01
        assert np.array_equal(got.alpha_index[s][decided], ref.alpha_index[s][decided])
        for a in np.unique(got.alpha_index[s]):
            cols = got.alpha_index[s] == a
            err = np.abs(got.weights[s].astype(np.float64) - ref.weights[s].astype(np.float64))
            assert (err <= ec.weights_bound(feats, mem, alphas[a], yard['weights'][a]))[:, cols].all()
    record_measured('ridge_cv_vs_host', duplicate=bool(duplicate), kind=kind, fraction_of_bound=used)
    used = ec.check_result(got, duplicate, kind)                # (and against the explicit route itself)
    record_measured('ridge_cv_vs_yardstick', duplicate=bool(duplicate), kind=kind, fraction_of_bound=used)


def test_shared_alpha_and_explicit_folds(plain):
    got = device(alpha='shared')
    ec.check_result(got, False, 'r2', shared=True)
    same_bits(got._replace(score=plain.score, alpha_index=plain.alpha_index, weights=plain.weights), plain, 'the table under shared')
    ref = ridge_cv_host(list(ec.data()[0]), list(ec.data()[1]), ec.ALPHAS, groups=ec.GROUPS, alpha='shared')
    assert np.array_equal(got.alpha_index, ref.alpha_index)
    folds = [[[0, 1], [2]], [[3, 0], [1, 2]]]
    got = device(folds=folds)
    assert got.folds == [[[0, 1], [2]], [[0, 3], [1, 2]]]
    ec.check_result(got, False, 'r2', folds=got.folds)
    bare = device(weights=False, scores=False)
    assert bare.weights is None and bare.scores is None
    assert np.array_equal(bare.score, plain.score) and np.array_equal(bare.alpha_index, plain.alpha_index)


@pytest.mark.parametrize('batch_runs', [1, 2])
def test_bit_identical_under_batching(plain, batch_runs):
    same_bits(device(batch_runs=batch_runs), plain, 'batch_runs = %d' % batch_runs)


def test_bit_identical_under_a_permutation_of_the_subjects(plain):
    runs, feats = ec.data()
    order = [3, 4, 0, 5, 1, 6, 2]
    got = ridge_cv([runs[r] for r in order], [feats[r] for r in order], ec.ALPHAS, groups=[ec.GROUPS[r] for r in order], scores=True)
    assert got.groups == ['b', 'a']
    same_bits(got._replace(**{n: getattr(got, n)[::-1].copy() for n in MAPS}), plain, 'subjects permuted')


def test_bit_identical_across_the_chunk_edge():
    """F = 64 fills one call of the statistics with the ones column in a second; a 65th feature that is zero moves the edge."""
    runs, feats = ec.data()
    rng = np.random.RandomState(11)
    f64 = [np.concatenate([x, rng.randn(x.shape[0], 64 - ec.F)], axis=1) for x in feats]
    f65 = [np.concatenate([x, np.zeros((x.shape[0], 1))], axis=1) for x in f64]
    _lib.dispatch_log = log = []
    try:
        a = ridge_cv(list(runs), f64, ec.ALPHAS, groups=ec.GROUPS, scores=True, batch_runs=4)
        n64 = len(log)
        b = ridge_cv(list(runs), f65, ec.ALPHAS, groups=ec.GROUPS, scores=True, batch_runs=4)
    finally:
        _lib.dispatch_log = None
    p16 = ' + '.join(['glm_project_kernel<16>'] * 4)                  # (64 columns: four panels of 16)
    tail = [('ridge_rotate', 'ridge_rotate_kernel'), ('ridge_score', 'ridge_score_kernel<%d> + ridge_select_kernel'),
            ('ridge_weights', 'ridge_weights_kernel')]
    want64 = [('glm_project', p16), ('glm_project', 'glm_project_kernel<1>')] + [(w, k % 64 if '%' in k else k) for w, k in tail]
    want65 = [('glm_project', p16), ('glm_project', 'glm_project_kernel<2>')] + [(w, k % 128 if '%' in k else k) for w, k in tail]
    assert log[:n64] == want64 * 2 and log[n64:] == want65 * 2
    assert (b.weights[:, 64] == 0).all()
    same_bits(b._replace(weights=np.ascontiguousarray(b.weights[:, :64])), a, 'a null 65th feature')


def test_tensors_in_tensors_out(plain):
    runs, feats = ec.data()
    got = ridge_cv([torch.as_tensor(np.array(r)).to(DEV) for r in runs], list(feats), ec.ALPHAS, groups=ec.GROUPS, scores=True)
    for name in MAPS:
        t = getattr(got, name)
        assert torch.is_tensor(t) and t.device == DEV
    same_bits(got, plain, 'tensor input')
    X = feats[1]
    pred = got.predict(X, 'a')
    assert torch.is_tensor(pred) and pred.dtype == torch.float32
    ref = plain.predict(X, 'a')
    assert np.abs(pred.cpu().numpy() - ref).max() <= 2.0 ** -22 * np.abs(ref).max()
    mixed = ridge_cv([torch.as_tensor(np.array(runs[0])).to(DEV)] + list(runs[1:]), list(feats), ec.ALPHAS, groups=ec.GROUPS, scores=True)
    assert isinstance(mixed.score, np.ndarray)
    same_bits(mixed, plain, 'mixed input')


def test_dispatch_sequence_and_non_finite_input(plain):
    runs, feats = ec.data()
    _lib.dispatch_log = log = []
    try:
        device(batch_runs=2)
    finally:
        _lib.dispatch_log = None
    project = ' + '.join(['glm_project_kernel<16>'] * 2 + ['glm_project_kernel<9>'])       # (F + 1 = 41 columns: one call)
    tail = [('ridge_rotate', 'ridge_rotate_kernel'), ('ridge_score', 'ridge_score_kernel<64> + ridge_select_kernel'),
            ('ridge_weights', 'ridge_weights_kernel')]
    assert log == [('glm_project', project)] * 2 + tail + [('glm_project', project)] * 2 + tail
    bad = [torch.as_tensor(np.array(r)).to(DEV) for r in runs]
    bad[5][3, 3] = float('nan')
    with pytest.raises(ValueError, match='ridge_cv: series hold non-finite values'):
        ridge_cv(bad, list(feats), ec.ALPHAS, groups=ec.GROUPS)
