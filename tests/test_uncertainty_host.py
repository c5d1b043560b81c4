"""Monte-Carlo dropout on the host: the mask's NumPy restatement against the header's formula written out in Python integers,
its threshold rule and kept share, ``mc_host`` / ``mc_measures`` against closed forms, every refusal of ``predict_mc`` and
``decode_series(mc=...)`` (raised before any device work, on a shape-only model), and the error codes of the two new entry
points.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from gcn_fmri_decoding_amd import _lib, graph as graph_mod, models_gcn, series, uncertainty

HEADER = open(os.path.join(ROOT, 'include', 'chebgcn.h')).read()
EINVAL, EUNSUPPORTED = -1, -4


def _constants():
    c = {k: int(v, 16) for k, v in re.findall(r'#define CHEBGCN_AUG_(\w+) (0x[0-9A-Fa-f]+)u', HEADER)}
    c['SITES'] = int(re.search(r'#define CHEBGCN_MC_SITES (\d+)', HEADER).group(1))
    return c


def _keep_scalar(seed, sample, layer, window, feature, keep):
    """The header's mask rule once more, in Python integers, with the constants parsed from the header."""
    c = _constants()

    def fin(x):
        x ^= x >> 16
        x = (x * c['MUL1']) & 0xFFFFFFFF
        x ^= x >> 15
        x = (x * c['MUL2']) & 0xFFFFFFFF
        return x ^ (x >> 16)
    refill = (sample * c['SITES'] + layer) & 0xFFFFFFFF
    i = window & 0xFFFFFFFF
    a = fin((fin(seed) + refill) & 0xFFFFFFFF)
    k0 = fin((a + i) & 0xFFFFFFFF)
    k1 = fin(((a ^ c['KEY']) + i * c['WINDOW']) & 0xFFFFFFFF)
    u = fin(fin((k0 + feature) & 0xFFFFFFFF) ^ k1)
    return u < min(int(keep * 2 ** 32), 2 ** 32 - 1)


# ------------------------------------------------------------------------------------------------ the mask

def test_mask_is_the_header_formula():
    assert _constants()['SITES'] == 16 == uncertainty.MC_SITES == _lib.MC_SITES
    windows = [0, 1, 7, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1, -1, -5]
    for seed, sample, layer, keep in [(0, 0, 0, 0.5), (12345, 3, 1, 0.8), (2 ** 32 - 1, 1023, 15, 0.25), (7, 31, 2, 0.5)]:
        got = uncertainty.dropout_keep(seed, sample, layer, windows, 37, keep)
        assert got.dtype == np.bool_ and got.shape == (len(windows), 37)
        want = np.array([[_keep_scalar(seed, sample, layer, w, d, keep) for d in range(37)] for w in windows])
        assert np.array_equal(got, want), (seed, sample, layer, keep)
    # the window number enters modulo 2^32: a negative int32 and its unsigned reading are the same window
    assert np.array_equal(uncertainty.dropout_keep(1, 2, 0, [-1], 64, 0.5), uncertainty.dropout_keep(1, 2, 0, [2 ** 32 - 1], 64, 0.5))
    # ... and the mask is a function of the window, not of its place in the list
    a = uncertainty.dropout_keep(5, 1, 0, [3, 9, 4], 50, 0.5)
    b = uncertainty.dropout_keep(5, 1, 0, [4, 3], 50, 0.5)
    assert np.array_equal(a[0], b[1]) and np.array_equal(a[2], b[0])
    # samples, sites and seeds draw different masks
    base = uncertainty.dropout_keep(5, 1, 0, np.arange(8), 256, 0.5)
    for other in (uncertainty.dropout_keep(5, 2, 0, np.arange(8), 256, 0.5), uncertainty.dropout_keep(5, 1, 1, np.arange(8), 256, 0.5),
                  uncertainty.dropout_keep(6, 1, 0, np.arange(8), 256, 0.5)):
        assert 0.3 < (base != other).mean() < 0.7
    with pytest.raises(ValueError, match='site'):
        uncertainty.dropout_keep(0, 0, 16, [0], 4, 0.5)


def test_threshold_rule():
    T, inv = uncertainty.dropout_threshold(0.5)
    assert T == 2 ** 31 and inv == np.float32(2.0) and isinstance(inv, np.float32)
    assert uncertainty.dropout_threshold(2.0 ** -32)[0] == 1
    assert uncertainty.dropout_threshold(2.0 ** -32 * (1 - 2.0 ** -53))[0] == 0          # just below one step: nothing is kept
    assert uncertainty.dropout_threshold(3 * 2.0 ** -32)[0] == 3
    assert uncertainty.dropout_threshold(1 - 2.0 ** -32)[0] == 2 ** 32 - 1
    assert uncertainty.dropout_threshold(np.nextafter(1.0, 0.0))[0] == 2 ** 32 - 1
    assert int(1.0 * 2 ** 32) == 2 ** 32 and uncertainty.dropout_threshold(1.0)[0] == 2 ** 32 - 1   # clamped into a uint32
    assert uncertainty.dropout_threshold(0.8)[1] == np.float32(1.0 / 0.8)
    for bad in (0.0, -0.1, 1.5, float('nan')):
        with pytest.raises(ValueError, match='keep'):
            uncertainty.dropout_threshold(bad)
    # the comparison itself, on the draws: u < T
    u = series.aug_draw(3, 5 * 16 + 1, np.arange(4, dtype=np.uint64)[:, None], np.arange(100, dtype=np.uint64)[None, :])
    for keep in (0.5, 0.8, 2.0 ** -32, 1.0):
        T = uncertainty.dropout_threshold(keep)[0]
        assert np.array_equal(uncertainty.dropout_keep(3, 5, 1, np.arange(4), 100, keep), u < T)
    assert not uncertainty.dropout_keep(3, 5, 1, np.arange(4), 100, 2.0 ** -32 * 0.5).any()


@pytest.mark.parametrize('seed', [0, 1, 0xDEADBEEF])
@pytest.mark.parametrize('keep', [0.5, 0.8, 0.1])
def test_kept_share_is_within_five_sigma(seed, keep):
    n = 2 ** 16
    m = uncertainty.dropout_keep(seed, 2, 1, np.arange(64), n // 64, keep)
    assert m.size == n
    sigma = np.sqrt(keep * (1 - keep) / n)
    assert abs(m.mean() - keep) <= 5 * sigma, (m.mean(), keep, sigma)
    # the reference stays inside too: NumPy's own generator at the same size
    ref = np.random.RandomState(seed % (2 ** 31)).rand(n) < keep
    assert abs(ref.mean() - keep) <= 5 * sigma


# ------------------------------------------------------------------------------------------------ the reduction and the host head

def _variables(rs, sizes):
    P = {}
    names = ['fc%d' % (i + 1) for i in range(len(sizes) - 2)] + ['logits']
    for name, I, O in zip(names, sizes[:-1], sizes[1:]):
        P[name + '/weights'] = rs.randn(I, O)
        P[name + '/bias'] = rs.randn(O)
    return P


def test_mc_host_one_sample_has_no_disagreement():
    rs = np.random.RandomState(0)
    P = _variables(rs, [7, 8, 6, 5])
    assert uncertainty.head_layers(P) == ['fc1', 'fc2', 'logits']
    r = uncertainty.mc_host(rs.randn(9, 7), P, np.arange(9), 1, 3, 0.5)
    assert r['logits'].shape == (1, 9, 5)
    assert np.array_equal(r['mutual_information'], np.zeros(9)) and np.array_equal(r['agreement'], np.ones(9))
    assert np.array_equal(r['entropy'], r['expected_entropy']) and (r['entropy'] > 0).all()
    assert np.array_equal(r['votes'].sum(axis=1), np.ones(9)) and r['votes'].dtype == np.int32
    assert np.array_equal(r['labels'], np.argmax(r['logits'][0], axis=1)) and r['labels'].dtype == np.int64
    assert np.allclose(r['probabilities'].sum(axis=1), 1.0, atol=1e-14)


def test_mc_host_is_the_masked_head_written_out():
    rs = np.random.RandomState(1)
    P = _variables(rs, [4, 6, 5, 3])
    f = rs.randn(3, 4)
    windows = np.array([11, 2 ** 31 + 5, 4])
    r = uncertainty.mc_host(f, P, windows, 4, 9, 0.8)
    h1 = np.maximum(f @ P['fc1/weights'] + P['fc1/bias'], 0.0)
    scale = np.float64(np.float32(1.0 / 0.8))
    for s in range(4):
        for w in range(3):
            m0 = np.array([_keep_scalar(9, s, 0, int(windows[w]), d, 0.8) for d in range(6)])
            h2 = np.maximum((h1[w] * m0 * scale) @ P['fc2/weights'] + P['fc2/bias'], 0.0)
            m1 = np.array([_keep_scalar(9, s, 1, int(windows[w]), d, 0.8) for d in range(5)])
            z = (h2 * m1 * scale) @ P['logits/weights'] + P['logits/bias']
            assert np.allclose(r['logits'][s, w], z, rtol=0, atol=1e-13)
    # more samples: the first ones stay what they were (a sample is a function of its number)
    r2 = uncertainty.mc_host(f, P, windows, 6, 9, 0.8)
    assert np.array_equal(r2['logits'][:4], r['logits'])
    assert (r2['mutual_information'] >= 0).all()
    with pytest.raises(ValueError, match='hidden'):
        uncertainty.mc_host(f, {'logits/weights': rs.randn(4, 3), 'logits/bias': rs.randn(3)}, windows, 2, 0, 0.5)


def test_measures_closed_forms():
    # two identical logit columns tie to the first -- votes, labels
    z = np.zeros((3, 2, 4))
    z[:, 0] = [1.0, 2.0, 2.0, 0.0]
    z[:, 1] = [0.5, 0.5, 0.5, 0.5]
    r = uncertainty.mc_measures(z)
    assert r['labels'].tolist() == [1, 0] and r['votes'].tolist() == [[0, 3, 0, 0], [3, 0, 0, 0]]
    assert r['agreement'].tolist() == [1.0, 1.0]
    assert np.isclose(r['entropy'][1], np.log(4)) and np.isclose(r['expected_entropy'][1], np.log(4))
    assert r['mutual_information'][1] == 0.0
    # saturated logits: entropy 0, not NaN
    z = np.full((2, 1, 3), -800.0)
    z[:, 0, 2] = 800.0
    r = uncertainty.mc_measures(z)
    assert r['entropy'][0] == 0.0 and r['expected_entropy'][0] == 0.0 and r['mutual_information'][0] == 0.0
    assert r['probabilities'][0].tolist() == [0.0, 0.0, 1.0] and r['labels'][0] == 2
    # two samples that are sure of different classes: all of the uncertainty is mutual information (0 log 0 = 0 throughout)
    z[0, 0] = [900.0, -900.0, 0.0]
    r = uncertainty.mc_measures(z)
    assert np.isfinite(r['entropy'][0]) and np.isclose(r['entropy'][0], np.log(2)) and r['expected_entropy'][0] == 0.0
    assert np.isclose(r['mutual_information'][0], np.log(2)) and r['agreement'][0] == 0.5 and r['labels'][0] == 0
    # a NaN counts as the largest value for the votes (the first one wins)
    z = np.array([[[0.0, np.nan, 5.0, np.nan]], [[1.0, 3.0, 3.0, 0.0]]])
    r = uncertainty.mc_measures(z)
    assert r['votes'].tolist() == [[0, 2, 0, 0]] and np.isnan(r['entropy'][0]) and np.isnan(r['mutual_information'][0])
    # C = 1: nothing to be unsure of
    r = uncertainty.mc_measures(np.random.RandomState(0).randn(5, 3, 1))
    assert not r['entropy'].any() and not r['mutual_information'].any() and (r['agreement'] == 1).all()


# ------------------------------------------------------------------------------------------------ refusals

def _meta_model(cls=models_gcn.cgcnn, M=(8, 5), **kw):
    Ls = graph_mod.synthetic_graph(60, k=4, levels=0, seed=1)[0]
    return cls({'device': 'meta'}, Ls * 2, [4, 4], [3, 3], [1, 1], list(M), channel=3, batch_size=4, verbose=False, **kw)


X = np.zeros((6, 60, 3), np.float32)
BAD = [
    (dict(samples=0), 'samples'), (dict(samples=1025), 'samples'), (dict(samples=2.0), 'samples'), (dict(samples=True), 'samples'),
    (dict(seed=-1), 'seed'), (dict(seed=2 ** 32), 'seed'), (dict(seed=1.5), 'seed'),
    (dict(keep=0.0), 'keep'), (dict(keep=1.0), 'keep'), (dict(keep=1), 'keep'), (dict(keep=-0.5), 'keep'), (dict(keep='half'), 'keep'),
    (dict(keep=float('nan')), 'keep'),
    (dict(batch_size=0), 'batch_size'), (dict(batch_size=70000), 'batch_size'), (dict(batch_size=2.5), 'batch_size'),
]


@pytest.mark.parametrize('kw,word', BAD)
def test_predict_mc_arguments_raise_before_device_work(kw, word):
    net = _meta_model(dropout=0.5)
    with pytest.raises(ValueError, match=word):
        net.predict_mc(X, **kw)
    if 'batch_size' not in kw:
        with pytest.raises(ValueError, match=word):
            net.decode_series(np.zeros((20, 60), np.float32), mc=kw)


def test_predict_mc_refusals():
    net = _meta_model(dropout=0.5)
    with pytest.raises(ValueError, match='data'):
        net.predict_mc(np.zeros((6, 59, 3), np.float32))
    with pytest.raises(ValueError, match='data'):
        net.predict_mc(np.zeros((0, 60, 3), np.float32))
    # keep not given and the model's dropout outside (0, 1)
    for d in (1, 1.0, 0):
        with pytest.raises(ValueError, match='dropout'):
            _meta_model(dropout=d).predict_mc(X)
        with pytest.raises(ValueError, match='dropout'):
            _meta_model(dropout=d).decode_series(np.zeros((20, 60), np.float32), mc={})
    # no hidden FC layer: no dropout site
    with pytest.raises(ValueError, match='hidden FC layer'):
        _meta_model(M=(5,), dropout=0.5).predict_mc(X)
    with pytest.raises(ValueError, match='classes'):
        _meta_model(M=(8, 65), dropout=0.5).predict_mc(X)
    with pytest.raises(ValueError, match='mc must be a dict'):
        net.decode_series(np.zeros((20, 60), np.float32), mc=dict(sample=3))
    with pytest.raises(ValueError, match='mc must be a dict'):
        net.decode_series(np.zeros((20, 60), np.float32), mc=32)
    # everything in order: a shape-only model has no device to run on (decode_series' rule)
    with pytest.raises(RuntimeError, match='device'):
        net.predict_mc(X)
    with pytest.raises(RuntimeError, match='device'):
        _meta_model(dropout=1).predict_mc(X, keep=0.5, samples=1024, seed=2 ** 32 - 1, batch_size=7, return_samples=True)
    with pytest.raises(RuntimeError, match='device'):
        net.decode_series(np.zeros((20, 60), np.float32), mc=dict(samples=4, seed=1, keep=0.9))
    assert net._mc is None


def test_finetuning_model_refuses():
    """Both public entries of a fine-tuning model refuse, after their argument checks and before the device is asked for.  (A
    shape-only finetuning_cgcnn needs a checkpoint to build from; the entries read only the attributes set here before they
    refuse.  tests/test_gpu_uncertainty.py repeats this on a real model.)"""
    ft = object.__new__(models_gcn.finetuning_cgcnn)
    ft._M0, ft.channel, ft.batch_size, ft.dropout, ft.M = 60, 3, 4, 0.5, [8, 5]
    with pytest.raises(NotImplementedError, match='never drops out'):
        ft.predict_mc(X)
    with pytest.raises(NotImplementedError, match='never drops out'):
        ft.decode_series(np.zeros((20, 60), np.float32), mc=dict(samples=4))
    with pytest.raises(ValueError, match='samples'):                       # the argument checks come first
        ft.predict_mc(X, samples=0)


# ------------------------------------------------------------------------------------------------ ABI

def test_entry_points_refuse_bad_arguments_without_a_gpu():
    lib = _lib.lib()
    for name in ('chebgcn_fc_fwd_dropout', 'chebgcn_fc_fwd_dropout_supported', 'chebgcn_fc_fwd_dropout_workspace', 'chebgcn_mc_reduce',
                 'chebgcn_mc_reduce_supported'):
        assert name in _lib.SIGNATURES and re.search(r'\b%s\s*\(' % name, HEADER)
    sup, ws = lib.chebgcn_fc_fwd_dropout_supported, lib.chebgcn_fc_fwd_dropout_workspace
    assert sup(1, 1, 1, 1) == 1 and sup(32, 128, 512, 256) == 1 and sup(4, 512, 16, 512) == 1
    assert sup(0, 1, 1, 1) == 0 and sup(1, 0, 1, 1) == 0 and sup(1, 1, 0, 1) == 0 and sup(1, 1, 1, 0) == 0
    assert sup(5, 512, 16, 512) == 0 and sup(1, 1, (1 << 20) + 1, 1) == 0 and sup(32769, 1, 1, 1) == 0
    assert ws(1, 1, 512, 1) == 0 and ws(1, 1, 513, 1) == 2 * 4 and ws(3, 1, 513, 1) == 2 * 3 * 4
    assert ws(3, 33, 10466, 40) == 21 * 3 * 33 * 40 * 4                  # 512 // (3 * 2 * 2) = 42 splits at most, 21 lengths of 512
    assert ws(32, 128, 512, 256) == 0 and ws(0, 1, 1, 1) == 0
    one = ctypes.c_void_p(16)                                             # never dereferenced: every call below is refused first

    def fc(x=one, ldx=4, sx=0, W=one, y=one, win=one, S=1, B=1, I=4, O=1, s0=0, layer=0, inv_keep=2.0):
        return lib.chebgcn_fc_fwd_dropout(x, ldx, sx, W, None, y, None, 0, win, S, B, I, O, 0, 0, s0, layer, 1 << 31, inv_keep, None)
    for kw in (dict(x=None), dict(W=None), dict(y=None), dict(win=None), dict(S=0), dict(B=0), dict(I=0), dict(O=0), dict(ldx=3),
               dict(sx=2, B=2, ldx=4), dict(s0=-1), dict(layer=-1), dict(layer=16), dict(inv_keep=0.5), dict(inv_keep=float('inf')),
               dict(inv_keep=float('nan'))):
        assert fc(**kw) == EINVAL and b'fc_fwd_dropout' in lib.chebgcn_last_error(), kw
    for kw in (dict(ldx=6, I=5), dict(x=ctypes.c_void_p(20)), dict(sx=6, I=4, ldx=4), dict(S=5, B=512, O=512), dict(S=40000)):
        assert fc(**kw) == EUNSUPPORTED, kw
    assert fc(I=513, ldx=516) == EINVAL and b'workspace' in lib.chebgcn_last_error()
    msup = lib.chebgcn_mc_reduce_supported
    assert msup(1, 1) == 1 and msup(1024, 64) == 1 and msup(1025, 64) == 0 and msup(4, 65) == 0 and msup(0, 4) == 0 and msup(4, 0) == 0

    def red(z=one, S=2, B=1, C=3, outs=(one,) * 7):
        return lib.chebgcn_mc_reduce(z, S, B, C, *outs, None)
    for kw in (dict(z=None), dict(S=0), dict(B=0), dict(C=0), dict(outs=(one,) * 6 + (None,)), dict(outs=(None,) + (one,) * 6)):
        assert red(**kw) == EINVAL and b'mc_reduce' in lib.chebgcn_last_error(), kw
    assert red(S=1025) == EUNSUPPORTED and red(C=65) == EUNSUPPORTED
