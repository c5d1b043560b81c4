"""Shapley maps (base_model.shapley / shapley_maps) on the host: the permutation table of a call, the float64 restatement
``shapley_host`` the GPU tests compare against -- checked here on an additive game, where every permutation gives the exact
answer, and against the closed-form coalition formula on three groups -- and the argument checks of the public methods, which
raise before any device work (on a shape-only model).  No GPU."""
import itertools
import math

import numpy as np
import pytest

from gcn_fmri_decoding_amd import _lib, attribution
from gcn_fmri_decoding_amd import graph as graph_mod
from gcn_fmri_decoding_amd import models_gcn


def shapley_host(f, x, groups, baseline, perms):
    """phi [S, G] in float64 of windows ``x`` [S, M, C] for any callable ``f``: rows [R, M, C] -> scores [R].  ``groups``:
    int [M] in [-1, G) (None: one group per vertex), ``baseline``: [M, C] or None (zeros), ``perms``: int [P, G].  Per window
    and permutation, the G + 1 rows of the definition: row j has the window's values on the first j groups of the permutation
    (and on group -1), the baseline elsewhere; phi[w, g] is the mean over the permutations of f(row pos(g) + 1) - f(row pos(g))."""
    x = np.asarray(x, np.float64)
    S, M, C = x.shape
    g = np.arange(M) if groups is None else np.asarray(groups, np.int64)
    perms = np.asarray(perms, np.int64)
    P, G = perms.shape
    assert G == int(g.max()) + 1
    x0 = np.zeros((M, C)) if baseline is None else np.asarray(baseline, np.float64)
    phi = np.zeros((S, G))
    for w in range(S):
        for p in range(P):
            rows = np.repeat(x0[None], G + 1, axis=0)
            rows[:, g < 0] = x[w][g < 0]
            for j in range(G):
                rows[j + 1:, g == perms[p, j]] = x[w][g == perms[p, j]]
            s = np.asarray(f(rows), np.float64)
            phi[w, perms[p]] += s[1:] - s[:-1]
    return phi / P


# ------------------------------------------------------------------------------------ the permutation table

@pytest.mark.parametrize('G,P', [(1, 1), (2, 2), (7, 5), (7, 16), (300, 3)])
@pytest.mark.parametrize('antithetic', [False, True])
def test_permutation_table(G, P, antithetic):
    state = np.random.get_state()
    t = attribution.shapley_permutations(G, P, antithetic, 11)
    after = np.random.get_state()
    assert state[0] == after[0] and np.array_equal(state[1], after[1]) and state[2:] == after[2:]
    assert t.dtype == np.int32 and t.shape == (P, G)
    assert np.array_equal(np.sort(t, axis=1), np.broadcast_to(np.arange(G), (P, G)))
    if antithetic:
        for i in range(P // 2):
            assert np.array_equal(t[2 * i + 1], t[2 * i][::-1])
    assert np.array_equal(t, attribution.shapley_permutations(G, P, antithetic, 11))
    # the drawn rows are RandomState(seed).permutation(G), one after the other
    rs = np.random.RandomState(11)
    drawn = t[::2] if antithetic else t
    assert np.array_equal(drawn, np.stack([rs.permutation(G) for _ in range(len(drawn))]))
    if G >= 7:
        assert not np.array_equal(t, attribution.shapley_permutations(G, P, antithetic, 12))


# ------------------------------------------------------------------------------------ the restatement

def _game(seed=0, S=3, M=20, C=2, G=5, holes=True):
    rs = np.random.RandomState(seed)
    x, base = rs.randn(S, M, C), rs.randn(M, C)
    groups = rs.randint(-1 if holes else 0, G, M)
    groups[:G] = np.arange(G)
    return rs, x, base, groups


@pytest.mark.parametrize('antithetic', [False, True])
def test_additive_game_is_exact_for_every_table(antithetic):
    rs, x, base, groups = _game()
    a = rs.randn(*x.shape[1:])
    for P, seed in ((1, 0), (3, 1), (8, 2)):
        perms = attribution.shapley_permutations(5, P, antithetic, seed)
        for b in (base, None):
            phi = shapley_host(lambda rows: (rows * a).sum(axis=(1, 2)), x, groups, b, perms)
            d = a * (x - (b if b is not None else 0.0))
            want = np.stack([d[:, groups == g].sum(axis=(1, 2)) for g in range(5)], axis=1)
            assert np.abs(phi - want).max() <= 1e-13 * np.abs(want).max()


def test_three_groups_all_permutations_equal_the_coalition_formula():
    rs, x, base, groups = _game(seed=4, G=3)
    Wt = rs.randn(x.shape[1] * x.shape[2], 6)

    def f(rows):                                        # not additive: the groups interact
        return np.tanh(rows.reshape(len(rows), -1) @ Wt).prod(axis=1) + (rows ** 2).sum(axis=(1, 2))

    perms = np.array(list(itertools.permutations(range(3))), np.int32)
    phi = shapley_host(f, x, groups, base, perms)

    def v(w, coalition):
        row = base.copy()
        keep = (groups < 0) | np.isin(groups, list(coalition))
        row[keep] = x[w][keep]
        return float(f(row[None])[0])

    want = np.zeros((len(x), 3))
    for w in range(len(x)):
        for g in range(3):
            others = [k for k in range(3) if k != g]
            for n in range(3):
                for T in itertools.combinations(others, n):
                    weight = math.factorial(n) * math.factorial(3 - n - 1) / math.factorial(3)
                    want[w, g] += weight * (v(w, T + (g,)) - v(w, T))
    assert np.abs(phi - want).max() <= 1e-12 * np.abs(want).max()
    # efficiency, for any table
    one = shapley_host(f, x, groups, base, perms[4:5])
    total = np.array([v(w, (0, 1, 2)) - v(w, ()) for w in range(len(x))])
    assert np.abs(one.sum(axis=1) - total).max() <= 1e-12 * np.abs(total).max()


# ------------------------------------------------------------------------------------ the argument checks

_graph = {}


def _meta_model(channel=3, N=60):
    if N not in _graph:
        _graph[N] = graph_mod.synthetic_graph(N, k=4, levels=0, seed=1)[0]
    return models_gcn.cgcnn({'device': 'meta'}, _graph[N] * 2, [4, 4], [3, 3], [1, 1], [8, 5], channel=channel, batch_size=4,
                            verbose=False)


_holes = np.arange(60) % 4
_holes[_holes == 2] = 3                         # id 2 occurs nowhere
BAD = [
    (dict(permutations=0), 'permutations'),
    (dict(permutations=4097), 'permutations'),
    (dict(permutations=2.5), 'permutations'),
    (dict(permutations=True), 'permutations'),
    (dict(antithetic=1), 'antithetic'),
    (dict(seed=-1), 'seed'),
    (dict(seed=2 ** 32), 'seed'),
    (dict(groups=_holes), 'groups'),
    (dict(groups=np.arange(59)), 'groups'),
    (dict(groups=np.ones(60, bool)), 'groups'),
    (dict(groups=np.arange(60) - 2), 'groups'),
    (dict(groups=-np.ones(60, np.int64)), 'groups'),
    (dict(score='prob'), 'score'),
    (dict(baseline=np.zeros((60, 2))), 'baseline'),
    (dict(batch_size=0), 'batch_size'),
    (dict(batch_size=65536), 'batch_size'),
]


@pytest.mark.parametrize('kw,word', BAD)
def test_shapley_arguments_raise_before_device_work(kw, word):
    net = _meta_model()
    with pytest.raises(ValueError, match=word) as e:
        net.shapley(np.zeros((6, 60, 3), np.float32), **kw)
    assert str(e.value).startswith('shapley: ')
    with pytest.raises(ValueError, match=word):
        net.shapley_maps(np.zeros((6, 60, 3), np.float32), np.arange(6) % 5, **kw)


@pytest.mark.parametrize('kw,word', [(dict(target=5), 'target'), (dict(target='label'), 'labels'),
                                     (dict(target=np.arange(5)), 'target')])
def test_shapley_targets_are_checked(kw, word):
    with pytest.raises(ValueError, match=word):
        _meta_model().shapley(np.zeros((6, 60, 3), np.float32), **kw)


def test_more_than_4096_groups_are_refused():
    net = _meta_model(N=4097)
    x = np.zeros((1, 4097, 3), np.float32)
    with pytest.raises(ValueError, match='groups') as e:
        net.shapley(x)                                  # groups=None: one per vertex, G = 4097
    assert '4096' in str(e.value)
    with pytest.raises(RuntimeError, match='device'):
        net.shapley(x, groups=np.minimum(np.arange(4097), 4095))       # G = 4096 goes on to the device


def test_own_arguments_are_checked_before_groups_and_groups_before_the_shared_ones():
    net = _meta_model()
    x = np.zeros((6, 60, 3), np.float32)
    with pytest.raises(ValueError, match='permutations'):
        net.shapley(x, permutations=0, groups=_holes, score='prob')
    with pytest.raises(ValueError, match='groups'):
        net.shapley(x, groups=_holes, score='prob')


def test_valid_arguments_reach_the_device_check():
    """Arguments that pass every check go on to the device: a shape-only model has none to run on."""
    net = _meta_model()
    x = np.zeros((6, 60, 3), np.float32)
    with pytest.raises(RuntimeError, match='device'):
        net.shapley(x)
    with pytest.raises(RuntimeError, match='device'):
        net.shapley(x, target=np.arange(6) % 5, score='logprob', groups=np.arange(60) >> 3, baseline=np.ones((60, 3)),
                    permutations=4096, antithetic=False, seed=2 ** 32 - 1, batch_size=65535)
    with pytest.raises(RuntimeError, match='device'):
        net.shapley(x, target='label', labels=np.arange(6) % 5, permutations=np.int64(1),
                    groups=np.where(np.arange(60) < 10, -1, np.arange(60) % 4))
    with pytest.raises(RuntimeError, match='device'):
        net.shapley_maps(x, np.arange(6) % 5, groups=list(np.arange(60) % 6), permutations=3)


def test_channel_limit_is_checked_with_the_arguments():
    L = _lib.lib()
    assert L.chebgcn_shapley_supported(125) == 1
    assert L.chebgcn_shapley_supported(126) == 0
    assert L.chebgcn_shapley_supported(0) == 0
    with pytest.raises(ValueError, match='channels'):
        _meta_model(126).shapley(np.zeros((2, 60, 126), np.float32))
    with pytest.raises(RuntimeError, match='device'):
        _meta_model(125).shapley(np.zeros((2, 60, 125), np.float32))


def test_occlusion_messages_are_unchanged_by_the_shared_group_check():
    net = _meta_model()
    with pytest.raises(ValueError) as e:
        net.occlusion(np.zeros((6, 60, 3), np.float32), groups=np.arange(60) - 2)
    assert str(e.value) == 'occlusion: groups must lie in [-1, G) (-1: never occluded); got -2'
    with pytest.raises(ValueError) as e:
        net.occlusion(np.zeros((6, 60, 3), np.float32), groups=_holes)
    assert str(e.value) == 'occlusion: groups must use every id in [0, 4); 1 of them occur nowhere (first 2)'


# ------------------------------------------------------------------------------------ the kernel test's row restatement

def test_row_restatement_of_the_kernel_tests_is_the_literal_definition():
    """``ref_shapley_rows`` (what tests/test_gpu_shapley_kernels.py holds the row kernel to, vectorised) against nested loops
    that transcribe the header's contract element by element."""
    from test_gpu_shapley_kernels import plane_stride, ref_shapley_rows
    rs = np.random.RandomState(8)
    S, N, M, F, G, P = 2, 9, 11, 2, 3, 2
    Mp = plane_stride(M)
    x, x0 = rs.randn(S, N, F).astype(np.float32), rs.randn(N, F).astype(np.float32)
    perm = rs.permutation(M).astype(np.int32)           # entries >= N: fake positions
    gid = rs.randint(-1, G, M).astype(np.int32)
    gid[:G] = np.arange(G)
    perms = attribution.shapley_permutations(G, P, True, 0)
    rank = np.empty_like(perms)
    for p in range(P):
        for k in range(G):
            rank[p, perms[p, k]] = k
    r0, R = 3, S * P * (G + 1)                          # runs three rows past the last window
    for base in (None, x0):
        want = np.zeros((R, F, Mp), np.float32)
        for r in range(r0, r0 + R):
            w, p, j = r // (P * (G + 1)), (r // (G + 1)) % P, r % (G + 1)
            if w >= S:
                continue
            for i in range(M):
                if perm[i] >= N:
                    continue
                own = gid[i] < 0 or rank[p, gid[i]] < j
                for f in range(F):
                    want[r - r0, f, i] = x[w, perm[i], f] if own else (base[perm[i], f] if base is not None else 0.0)
        assert np.array_equal(ref_shapley_rows(x, perm, gid, rank, base, r0, R, M), want)
