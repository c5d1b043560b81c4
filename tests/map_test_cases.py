"""Graphs, maps and an independent restatement shared by the map_test tests (not a test module itself)."""
import math
from collections import deque

import numpy as np
import scipy.sparse as sp


def from_edges(M, pairs):
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    return sp.csr_matrix((np.ones(len(pairs), np.float32), (pairs[:, 0], pairs[:, 1])), shape=(M, M))


def path(M, numbering=None):
    """A path through all M vertices; ``numbering[k]`` is the vertex at place k along it (default: k)."""
    o = np.arange(M) if numbering is None else np.asarray(numbering)
    return from_edges(M, np.stack([o[:-1], o[1:]], 1))


def ring(M):
    return from_edges(M, [(i, (i + 1) % M) for i in range(M)]) if M > 2 else path(M)


def star(M, centre=0):
    return from_edges(M, [(centre, v) for v in range(M) if v != centre])


def two_components_with_isolated(M):
    """Two equal paths, and every fifth vertex isolated."""
    live = [v for v in range(M) if v % 5 != 4]
    half = len(live) // 2
    a, b = live[:half], live[half:2 * half]
    return from_edges(M, [(a[k], a[k + 1]) for k in range(half - 1)] + [(b[k], b[k + 1]) for k in range(half - 1)])


def random_graph(M, degree, seed):
    rs = np.random.RandomState(seed)
    n = max(1, M * degree // 2)
    return from_edges(M, np.stack([rs.randint(0, M, n), rs.randint(0, M, n)], 1))


def grid(n):
    idx = np.arange(n * n).reshape(n, n)
    return from_edges(n * n, np.concatenate([np.stack([idx[:, :-1].ravel(), idx[:, 1:].ravel()], 1),
                                             np.stack([idx[:-1].ravel(), idx[1:].ravel()], 1)]))


def smooth_maps(S, M, seed, A=None, effect=0.8):
    """Unit noise plus an effect on the first third of the vertices, averaged once over the neighbours when a graph is given (so
    that clusters form): float32 [S, M]."""
    rs = np.random.RandomState(seed)
    x = rs.randn(S, M)
    x[:, :max(1, M // 3)] += effect
    if A is not None:
        W = sp.csr_matrix(A)
        W = ((W + W.T) > 0).astype(np.float64) + sp.identity(M)
        x = (W @ x.T).T / np.asarray(W.sum(1)).ravel()[None, :]
    return np.ascontiguousarray(x, dtype=np.float32)


def neighbours(A):
    A = sp.coo_matrix(A)
    nb = [set() for _ in range(A.shape[0])]
    for r, c, d in zip(A.row, A.col, A.data):
        if r != c and d != 0:
            nb[r].add(int(c))
            nb[c].add(int(r))
    return nb


def components_bfs(active, nb):
    """label[v] = smallest vertex of v's component among the active vertices (-1: not active), size[v] its size."""
    M = len(active)
    label, size = [-1] * M, [0] * M
    for s in range(M):
        if not active[s] or label[s] >= 0:
            continue
        seen, todo = [s], deque([s])
        label[s] = s
        while todo:
            v = todo.popleft()
            for u in nb[v]:
                if active[u] and label[u] < 0:
                    label[u] = s
                    seen.append(u)
                    todo.append(u)
        for v in seen:
            size[v] = len(seen)
    return label, size


def enhance_python(u, nb, stat, threshold=None, step=None, E=0.5, H=2.0):
    """One map ``u`` (float32 [M]) -> (stat float64 [M], labels [M]) by breadth-first search and a double loop over heights and
    vertices, heights descending; the two tables come from ``np.power`` as the stated arithmetic has them."""
    M = len(u)
    if stat == 'max':
        return np.asarray(u, np.float64), [-1] * M
    if stat == 'extent':
        n, hf, hw, ep = 1, [0.0, np.float32(threshold)], [0.0, 1.0], np.arange(M + 1, dtype=np.float64)
    else:
        top = float(np.max(u))
        n = int(math.floor(top / step)) if top > 0 else 0
        h = np.arange(n + 1, dtype=np.float64) * step
        hf, hw, ep = h.astype(np.float32), np.power(h, H) * step, np.power(np.arange(M + 1, dtype=np.float64), E)
    acc = [0.0] * M
    labels = [-1] * M
    for i in range(n, 0, -1):
        label, size = components_bfs([bool(u[v] > hf[i]) for v in range(M)], nb)
        for v in range(M):
            if label[v] >= 0:
                acc[v] = acc[v] + float(ep[size[v]]) * float(hw[i])
        if i == 1:
            labels = label
    return np.array(acc, np.float64), labels
