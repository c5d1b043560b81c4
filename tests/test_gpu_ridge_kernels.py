"""The ridge kernels (chebgcn_ridge_rotate / _score / _weights) driven through the C ABI with synthetic float64 tables and compared
BIT FOR BIT with the NumPy restatement of their chains in ``encoding`` (plain float64 ``*`` and ``+`` in the stated order: no fma
to emulate) -- at the smallest shapes at which each arm can go wrong: F below, at and above a register block (16), a wave's share
and every bucket of the score kernel (64, 128, 256); M below, at and above a tile and on three tiles; 1, 2 and 32 penalties;
training lists of 1, 2 and 5 runs; two subjects with different numbers of folds in one call.  Every input plane holds NaN in its
pad columns [M, Mp), one vertex has tss = 0, one reciprocal row is zero, one run number is out of range; every output and the
workspace sit between guard bands and are pre-filled with a poison, twice (tests/guarded_buffers.py).
"""
import numpy as np
import pytest
import torch

from gcn_fmri_decoding_amd import _lib, encoding as en, ops
from guarded_buffers import FILLS, Guarded, bits

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
GEO = ops.ridge_geometry()
TILE = GEO['tile']
OK, EINVAL, EUNSUPPORTED = 0, -1, -4
R = 6
# (training list, held-out list) of the models: folds of subject 0, folds of subject 1, then the all-runs model of either.  Lists
# of 1, 2 and 5 runs; 99 and -3 are no runs and are skipped
MODELS = [([0], [1, 2]), ([1, 2], [0]), ([0, 1, 2, 4, 5], [3]), ([3, 99, 5], [4, -3]), ([4], [3, 5]),
          ([0, 1, 2], []), ([3, 4, 5], [])]
FOLD_PTR = [0, 2, 5]
ALL_MODEL = [5, 6]
EF, S = 5, 2


def tables(F, M, A, seed):
    rng = np.random.RandomState(seed)
    Mp = _lib.plane_stride(M)
    c = np.full((R, F, Mp), np.nan)
    c[:, :, :M] = rng.randn(R, F, M)
    tss = np.full((R, Mp), np.nan)
    tss[:, :M] = rng.rand(R, M) * F + 0.5
    tss[:, M // 2] = 0.0                                         # (a vertex constant in every run)
    E = len(MODELS)
    V = rng.randn(E, F, F) / np.sqrt(F)
    H = rng.randn(E, F, F)
    H = (H + H.transpose(0, 2, 1)) / 2
    d = rng.rand(E, A, F) + 0.1
    if A > 1:
        d[:, A // 2] = 0.0                                       # (a zero reciprocal row: every weight of that penalty is 0)
    d[:, :, F // 3] = 0.0                                        # (and a null direction)
    ptr, flat = en._lists(MODELS)
    return dict(c=c, tss=tss, V=V, H=H, d=d, ptr=ptr, flat=flat, Mp=Mp)


def expected(t, F, M, A, kind):
    c, tss = t['c'][:, :, :M], t['tss'][:, :M]
    E = len(MODELS)
    ws = np.zeros((E, 2, F, t['Mp']))
    fold = np.zeros((EF, A, t['Mp']))
    for e, (train, test) in enumerate(MODELS):
        ws[e, 0, :, :M], ws[e, 1, :, :M] = en.model_chains(c, train, test, t['V'][e])
        if e < EF:
            fold[e, :, :M] = en.score_chains(ws[e, 0, :, :M], ws[e, 1, :, :M], en._list_sum(tss, test), t['H'][e], t['d'][e], kind)
    score, index, scores = np.zeros((S, M), np.float32), np.zeros((S, M), np.int32), np.zeros((S, A, M), np.float32)
    weights = np.zeros((S, F, M), np.float32)
    for s in range(S):
        score[s], index[s], scores[s] = en.select_chains(fold[FOLD_PTR[s]:FOLD_PTR[s + 1], :, :M])
        e = ALL_MODEL[s]
        weights[s] = en.weight_chains(ws[e, 0, :, :M], np.ascontiguousarray(t['V'][e].T), t['d'][e], index[s])
    return dict(ws=ws, fold=fold, score=score, index=index, scores=scores, weights=weights)


def put(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a, dtype)).to(DEV)


def run_case(F, M, A, kind, fill, t, want_scores=True):
    """The three entries on guarded, poisoned buffers -> their outputs as host arrays, and the dispatch strings."""
    lib = _lib.lib()
    E, Mp = len(MODELS), t['Mp']
    dev = {k: put(t[k]) for k in ('c', 'tss', 'V', 'H', 'd', 'ptr', 'flat')}
    Vt = put(t['V'].transpose(0, 2, 1))
    nbytes = int(lib.chebgcn_ridge_workspace(E, F, M))
    assert nbytes == E * 2 * F * Mp * 8
    ws = Guarded((E, 2, F, Mp), 'float64', fill, DEV, align=8)
    fold = Guarded((EF, A, Mp), 'float64', fill, DEV, align=8)
    score = Guarded((S, M), 'float32', fill, DEV, align=4)
    index = Guarded((S, M), 'int32', fill, DEV, align=4)
    scores = Guarded((S, A, M), 'float32', fill, DEV, align=4)
    weights = Guarded((S, F, M), 'float32', fill, DEV, align=4)
    fold_ptr, all_model = put(FOLD_PTR, np.int32), put(ALL_MODEL, np.int32)
    nlist = int(t['flat'].size)
    names = []
    p = lambda x: x.data_ptr()  # noqa: E731
    assert lib.chebgcn_ridge_rotate(p(dev['c']), R, p(dev['ptr']), p(dev['flat']), nlist, p(dev['V']), E, F, M, ws.ptr, nbytes,
                                    None) == OK, lib.chebgcn_last_error()
    names.append(_lib.last_dispatch())
    assert lib.chebgcn_ridge_score(ws.ptr, nbytes, p(dev['tss']), R, p(dev['ptr']), p(dev['flat']), nlist, p(dev['H']), p(dev['d']),
                                   p(fold_ptr), E, EF, S, F, A, M, _lib.RIDGE_SCORES.index(kind), fold.ptr, score.ptr, index.ptr,
                                   scores.ptr if want_scores else None, None) == OK, lib.chebgcn_last_error()
    names.append(_lib.last_dispatch())
    assert lib.chebgcn_ridge_weights(ws.ptr, nbytes, p(Vt), p(dev['d']), p(all_model), index.ptr, E, S, F, A, M, weights.ptr,
                                     None) == OK, lib.chebgcn_last_error()
    names.append(_lib.last_dispatch())
    torch.cuda.synchronize()
    out = {}
    for name, g in (('ws', ws), ('fold', fold), ('score', score), ('index', index), ('scores', scores), ('weights', weights)):
        g.check('%s (F = %d, M = %d, A = %d)' % (name, F, M, A))
        out[name] = g.host()
    return out, names


def check_case(F, M, A, kind='r2', seed=0):
    t = tables(F, M, A, seed + 1000 * F + 10 * M + A)
    ref = expected(t, F, M, A, kind)
    assert np.isfinite(ref['fold']).all() and (ref['fold'][:, :, M // 2] == 0).all()
    if A > 1:
        assert (ref['fold'][:, A // 2] == 0).all()               # (no weights: rss = tss, and q = 0 has no correlation)
    bucket = 64 if F <= 64 else 128 if F <= 128 else 256
    for _, fill in FILLS:
        got, names = run_case(F, M, A, kind, fill, t)
        assert names == ['ridge_rotate_kernel', 'ridge_score_kernel<%d> + ridge_select_kernel' % bucket, 'ridge_weights_kernel']
        for name in ('ws', 'fold', 'score', 'index', 'scores', 'weights'):
            same = bits(got[name]) == bits(ref[name].astype(got[name].dtype))
            assert same.all(), '%s: %d of %d values differ (F = %d, M = %d, A = %d, %s)' % (name, (~same).sum(), same.size, F, M, A, kind)
    return ref


@pytest.mark.parametrize('F', [1, 2, 17, 64, 65, 129, 256])
def test_every_feature_count(F):
    check_case(F, 2 * TILE + 3, 2)


@pytest.mark.parametrize('M', [1, TILE - 1, TILE, TILE + 1, 2 * TILE + 3])
def test_every_tile_edge(M):
    check_case(17, M, 2)
    check_case(65, M, 1, kind='r')


@pytest.mark.parametrize('A', [1, 2, 32])
@pytest.mark.parametrize('kind', ['r2', 'r'])
def test_every_penalty_count(A, kind):
    ref = check_case(17, TILE + 1, A, kind)
    if A > 1:
        assert len(np.unique(ref['index'])) > 1                 # (the selection is exercised)


def test_scores_may_be_left_out_and_wrappers_agree():
    F, M, A = 33, TILE + 5, 3
    t = tables(F, M, A, 5)
    ref = expected(t, F, M, A, 'r2')
    got, _ = run_case(F, M, A, 'r2', FILLS[0][1], t, want_scores=False)
    assert np.array_equal(bits(got['score']), bits(ref['score'])) and np.array_equal(got['index'], ref['index'])
    assert (bits(got['scores']) == 0xFFFFFFFF).all()            # (untouched: the poison)
    _lib.dispatch_log = log = []
    try:
        ws, nbytes = ops.ridge_rotate(put(t['c']), put(t['ptr']), put(t['flat']), put(t['V']), M)
        score, index, table, fold = ops.ridge_score(ws, nbytes, put(t['tss']), put(t['ptr']), put(t['flat']), put(t['H']), put(t['d']),
                                                    put(FOLD_PTR, np.int32), M, EF, 'r2', scores=True)
        weights = ops.ridge_weights(ws, nbytes, put(t['V'].transpose(0, 2, 1)), put(t['d']), put(ALL_MODEL, np.int32), index, M)
    finally:
        _lib.dispatch_log = None
    assert log == [('ridge_rotate', 'ridge_rotate_kernel'), ('ridge_score', 'ridge_score_kernel<64> + ridge_select_kernel'),
                   ('ridge_weights', 'ridge_weights_kernel')]
    for name, a in (('score', score), ('index', index), ('scores', table), ('weights', weights), ('fold', fold)):
        assert np.array_equal(bits(a.cpu().numpy()), bits(got[name] if name != 'scores' else ref['scores'])), name


def test_indices_read_from_memory_are_clamped():
    """A model number out of range gives weights of zero, a selected index out of range is clamped, list and fold pointers out of
    range are cut: nothing read from memory is trusted."""
    lib = _lib.lib()
    F, M, A = 5, 70, 3
    t = tables(F, M, A, 9)
    ref = expected(t, F, M, A, 'r2')
    E, Mp = len(MODELS), t['Mp']
    ws = put(ref['ws'])
    nbytes = E * 2 * F * Mp * 8
    index = ref['index'].copy()
    index[0, :10], index[0, 10:20] = -7, 1000
    for fill_name, fill in FILLS:
        weights = Guarded((S, F, M), 'float32', fill, DEV, align=4)
        assert lib.chebgcn_ridge_weights(ws.data_ptr(), nbytes, put(t['V'].transpose(0, 2, 1)).data_ptr(), put(t['d']).data_ptr(),
                                         put([5, E], np.int32).data_ptr(), put(index).data_ptr(), E, S, F, A, M, weights.ptr, None) == OK
        torch.cuda.synchronize()
        weights.check('weights')
        got = weights.host()
        want = en.weight_chains(ref['ws'][5, 0, :, :M], np.ascontiguousarray(t['V'][5].T), t['d'][5], np.clip(index[0], 0, A - 1))
        assert np.array_equal(bits(got[0]), bits(want)) and (bits(got[1]) == 0).all()
    # list pointers beyond the list, a descending pair, fold pointers beyond Ef
    ptr = t['ptr'].copy()
    ptr[-1] = 10 ** 6                                            # (the last list is empty anyway: the clamp keeps it so)
    ptr[1], ptr[2] = ptr[2], ptr[1]                              # (descending: the held-out list of model 0 is empty)
    g = Guarded((E, 2, F, Mp), 'float64', FILLS[0][1], DEV, align=8)
    assert lib.chebgcn_ridge_rotate(put(t['c']).data_ptr(), R, put(ptr).data_ptr(), put(t['flat']).data_ptr(), int(t['flat'].size),
                                    put(t['V']).data_ptr(), E, F, M, g.ptr, nbytes, None) == OK
    torch.cuda.synchronize()
    g.check('workspace')
    got = g.host()
    n = int(t['flat'].size)
    cut = [t['flat'][min(max(a, 0), n):max(min(max(b, 0), n), min(max(a, 0), n))] for a, b in zip(ptr[:-1], ptr[1:])]
    assert list(cut[0]) == [0, 1, 2] and len(cut[1]) == 0 and list(cut[2]) == [1, 2, 1, 2] and len(cut[-1]) == 0
    for e in range(E):                                           # (a list is what its two pointers say, whatever the others do)
        z, g2 = en.model_chains(t['c'][:, :, :M], cut[2 * e], cut[2 * e + 1], t['V'][e])
        assert np.array_equal(bits(got[e, 0, :, :M]), bits(z)) and np.array_equal(bits(got[e, 1, :, :M]), bits(g2))
    assert (got[0, 1] == 0).all() and (got[:, :, :, M:] == 0).all()
    fold = put(ref['fold'])
    score = Guarded((S, M), 'float32', FILLS[1][1], DEV, align=4)
    idx = Guarded((S, M), 'int32', FILLS[1][1], DEV, align=4)
    assert lib.chebgcn_ridge_score(ws.data_ptr(), nbytes, put(t['tss']).data_ptr(), R, put(t['ptr']).data_ptr(), put(t['flat']).data_ptr(),
                                   int(t['flat'].size), put(t['H']).data_ptr(), put(t['d']).data_ptr(),
                                   put([3, 2, 99], np.int32).data_ptr(), E, EF, S, F, A, M, 0, fold.data_ptr(), score.ptr, idx.ptr, None,
                                   None) == OK
    torch.cuda.synchronize()
    score.check('score'), idx.check('index')
    want = en.select_chains(ref['fold'][2:EF, :, :M])
    assert (score.host()[0] == 0).all() and (idx.host()[0] == 0).all()          # (a descending pair: no folds)
    assert np.array_equal(bits(score.host()[1]), bits(want[0])) and np.array_equal(idx.host()[1], want[1])


def test_a_list_is_cut_at_its_limit():
    """64 runs of a list are summed, the 65th is not."""
    lib = _lib.lib()
    n = GEO['max_runs'] + 1
    rng = np.random.RandomState(3)
    c = rng.randn(n, 1, 32)
    flat = np.concatenate([np.arange(n), np.arange(n - 1)]).astype(np.int32)     # (model 0: 65 runs; model 1: the first 64)
    ptr = np.asarray([0, n, n, 2 * n - 1, 2 * n - 1], np.int32)
    V = np.ones((2, 1, 1))
    g = Guarded((2, 2, 1, 32), 'float64', FILLS[0][1], DEV, align=8)
    assert lib.chebgcn_ridge_rotate(put(c).data_ptr(), n, put(ptr).data_ptr(), put(flat).data_ptr(), int(flat.size), put(V).data_ptr(), 2, 1, 3,
                                    g.ptr, g.nbytes, None) == OK
    torch.cuda.synchronize()
    g.check('workspace')
    got = g.host()
    want = en._list_sum(c[:, :, :3], range(n - 1))
    assert np.array_equal(bits(got[0, 0, :, :3]), bits(want)) and np.array_equal(bits(got[1, 0, :, :3]), bits(want))
    assert (got[:, 1] == 0).all() and (got[:, :, :, 3:] == 0).all()


def test_limits_on_either_side():
    """The largest F, A, E and S are served; one more is CHEBGCN_EUNSUPPORTED, before any launch."""
    lib = _lib.lib()
    check_case(GEO['max_F'], 3, 1)
    check_case(3, 3, GEO['max_A'])
    big = GEO['max_models']
    buf = torch.zeros(4 * big + 64, dtype=torch.float64, device=DEV)
    ints = torch.zeros(2 * big + 64, dtype=torch.int32, device=DEV)
    ws = torch.empty(big * 2 * 32, dtype=torch.float64, device=DEV)
    b, i, w = buf.data_ptr(), ints.data_ptr(), ws.data_ptr()
    nb = ws.numel() * 8
    out = torch.empty(big * 4, dtype=torch.float32, device=DEV)
    index = torch.empty(big, dtype=torch.int32, device=DEV)
    fold = torch.empty(big * 32, dtype=torch.float64, device=DEV)
    o = out.data_ptr()
    assert lib.chebgcn_ridge_rotate(b, 1, i, i, 1, b, big, 1, 1, w, nb, None) == OK
    assert lib.chebgcn_ridge_score(w, nb, b, 1, i, i, 1, b, b, i, big, big, big, 1, 1, 1, 0, fold.data_ptr(), o, index.data_ptr(), None,
                                   None) == OK
    assert lib.chebgcn_ridge_weights(w, nb, b, b, i, index.data_ptr(), big, big, 1, 1, 1, o, None) == OK
    torch.cuda.synchronize()
    assert (ws.view(big, 2, 32) == 0).all() and (out[:big] == 0).all()
    for F, A, E, S_ in ((GEO['max_F'] + 1, 1, 1, 1), (1, GEO['max_A'] + 1, 1, 1), (1, 1, big + 1, 1), (1, 1, big, big + 1)):
        if A == 1 and S_ == 1:
            assert lib.chebgcn_ridge_rotate(b, 1, i, i, 1, b, E, F, 1, w, 1 << 40, None) == EUNSUPPORTED
        assert lib.chebgcn_ridge_score(w, 1 << 40, b, 1, i, i, 1, b, b, i, E, 1, S_, F, A, 1, 0, fold.data_ptr(), o, i, None,
                                       None) == EUNSUPPORTED
        assert lib.chebgcn_ridge_weights(w, 1 << 40, b, b, i, i, E, S_, F, A, 1, o, None) == EUNSUPPORTED
    assert lib.chebgcn_ridge_rotate(b, 1, i, i, 1, b, 1, 1, 1, w, 2 * 32 * 8 - 1, None) == EINVAL
    assert lib.chebgcn_ridge_rotate(b, 1, i, i, 1, b, 1, 1, 1, w + 4, 1 << 20, None) == EINVAL
