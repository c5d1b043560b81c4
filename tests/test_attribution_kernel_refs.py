"""The float64 references of tests/test_gpu_attribution_kernels.py against literal nested-loop transcriptions of the header
comments of csrc/saliency.hip, csrc/occlusion.hip and csrc/gradcam.hip, on one tiny shape each.  No GPU: this is what shows,
on any machine, that the vectorised references say what the headers say."""
import math

import numpy as np

import test_gpu_attribution_kernels as K

U = 2.0 ** -24


def _mp(M):
    return (M + 31) // 32 * 32


def test_path_coefficients_are_the_midpoints():
    for steps in (1, 2, 3, 5, 7, 32):
        a = K.path_coefficients(steps)
        assert a.dtype == np.float32
        exact = (np.arange(steps) + 0.5) / steps
        assert (np.abs(a.astype(np.float64) - exact) <= 2 * U * exact).all()      # 1 / steps and the product: two roundings


def test_gather_and_perm_data_ref():
    rs = np.random.RandomState(0)
    S, N, M, F = 3, 5, 7, 2
    x = rs.randn(S, N, F).astype(np.float32)
    perm = np.array([4, 6, 0, 2, 5, 1, 3])              # 5, 6: fake positions
    sample = [2, 0, 2]
    want = np.zeros((3, F, _mp(M)), np.float32)
    for s in range(3):
        for i in range(M):
            for f in range(F):
                if perm[i] < N:
                    want[s, f, i] = x[sample[s], perm[i], f]
    got = K.ref_perm_data(x, perm, np.array(sample), M)
    assert got.dtype == np.float32 and np.array_equal(got, want)
    assert np.array_equal(K.ref_gather(x, None, N)[:, :, :N], np.swapaxes(x, 1, 2))


def test_path_ref():
    rs = np.random.RandomState(1)
    S, N, M, F, nw, steps, R = 4, 5, 6, 2, 2, 3, 8
    x, x0 = rs.randn(S, N, F).astype(np.float32), rs.randn(N, F).astype(np.float32)
    perm = np.array([3, 5, 0, 4, 1, 2])                 # 5: a fake position
    sample = np.array([3, 1])
    for base in (None, x0):
        want = np.full((R, F, _mp(M)), 0.0)
        tb = np.zeros((R, F, _mp(M)))
        for w in range(nw):
            for j in range(steps):
                a = float(np.float32(np.float32(j) + np.float32(0.5)) * (np.float32(1) / np.float32(steps)))
                for i in range(M):
                    for f in range(F):
                        if perm[i] < N:
                            b = float(base[perm[i], f]) if base is not None else 0.0
                            xv = float(x[sample[w], perm[i], f])
                            want[w * steps + j, f, i] = b + a * (xv - b)
                            tb[w * steps + j, f, i] = 3 * U * (abs(b) + abs(a * (xv - b)))
        ref, bound = K.ref_path(x, perm, sample, base, steps, R, M)
        assert np.array_equal(ref, want) and np.allclose(bound, tb, rtol=1e-14, atol=0)
        assert not ref[nw * steps:].any() and not ref[:, :, M:].any() and not ref[:, :, 1].any()


def test_reduce_ref():
    rs = np.random.RandomState(2)
    M, F, nw, steps, S = 5, 2, 3, 4, 4
    dx = rs.randn(nw * steps + 1, F, _mp(M)).astype(np.float32)
    dx[:, :, M:] = np.nan
    x, x0 = rs.randn(S, M, F).astype(np.float32), rs.randn(M, F).astype(np.float32)
    order = np.array([2, 0, 4, 1, 3])
    sample = np.array([1, 3, 1])
    inv = float(np.float32(1) / np.float32(steps))
    for method in ('gradient', 'grad_x_input', 'integrated'):
        for absolute in (False, True):
            for base in (None, x0):
                for perm in (order, None):
                    want, wb = np.zeros((nw, M, F)), np.zeros((nw, M, F))
                    for w in range(nw):
                        for i in range(M):
                            v = perm[i] if perm is not None else i
                            for f in range(F):
                                g = sum(float(dx[w * steps + j, f, i]) for j in range(steps))
                                ga = sum(abs(float(dx[w * steps + j, f, i])) for j in range(steps))
                                xv = float(x[sample[w], v, f])
                                n = steps - 1
                                if method == 'grad_x_input':
                                    g, ga, n = xv * g, abs(xv) * ga, n + 1
                                elif method == 'integrated':
                                    d = xv - (float(base[v, f]) if base is not None else 0.0)
                                    g, ga, n = d * (g * inv), abs(d) * (ga * inv), n + 2 + (base is not None)
                                want[w, v, f] = abs(g) if absolute else g
                                wb[w, v, f] = n * U * ga
                    ref, bound = K.ref_reduce(dx, x, perm, sample, base, nw, steps, M, method, absolute)
                    assert np.allclose(ref, want, rtol=1e-14, atol=1e-300) and np.allclose(bound, wb, rtol=1e-14, atol=0)
    ref, bound = K.ref_reduce(dx, None, order, None, None, nw * steps, 1, M, 'gradient', False)
    assert not bound.any() and np.array_equal(ref[:, order, :], np.swapaxes(dx[:nw * steps, :, :M], 1, 2))


def test_class_sums_ref():
    rs = np.random.RandomState(3)
    nw, NF, C = 6, 4, 3
    rows = rs.randn(nw, NF).astype(np.float32)
    cls = np.array([2, 0, 2, 2, 0, 2])
    acc = rs.randn(C, NF)
    want = acc.copy()
    for k in range(C):
        for e in range(NF):
            s, any_ = 0.0, False
            for w in range(nw):
                if cls[w] == k:
                    s, any_ = s + float(rows[w, e]), True
            if any_:
                want[k, e] = acc[k, e] + s
    got = K.ref_class_sums(rows, cls, acc)
    assert np.array_equal(got, want) and np.array_equal(got[1], acc[1])


def test_occlusion_rows_ref():
    rs = np.random.RandomState(4)
    S, N, M, F, G = 2, 5, 6, 2, 3
    x, x0 = rs.randn(S, N, F).astype(np.float32), rs.randn(N, F).astype(np.float32)
    perm = np.array([3, 5, 0, 4, 1, 2])
    gid = np.array([0, 2, -1, 1, 0, 2])
    for base in (None, x0):
        for r0, R in ((0, 8), (3, 9)):
            want = np.zeros((R, F, _mp(M)), np.float32)
            for rr in range(R):
                r = r0 + rr
                w, j = r // (G + 1), r % (G + 1)
                g = G if j == 0 else j - 1
                if w >= S:
                    continue
                for i in range(M):
                    for f in range(F):
                        if perm[i] >= N:
                            continue
                        if gid[i] == g:
                            want[rr, f, i] = base[perm[i], f] if base is not None else 0.0
                        else:
                            want[rr, f, i] = x[w, perm[i], f]
            got = K.ref_occlusion_rows(x, perm, gid, base, r0, R, G, M)
            assert got.dtype == np.float32 and np.array_equal(got, want)


def test_score_ref():
    rs = np.random.RandomState(5)
    S, G, C = 3, 2, 4
    z = (rs.randn(S * (G + 1) + 2, C) * 8).astype(np.float32)
    cls = np.array([1, 3, 0])
    for score in ('logit', 'logprob'):
        want_ref, want = np.zeros(S), np.zeros((S, G))
        wb_ref, wb = np.zeros(S), np.zeros((S, G))

        def s_of(row, c):
            zz = [float(v) for v in row]
            if score == 'logit':
                return zz[c], 0.0
            m = max(zz)
            return (zz[c] - m) - math.log(sum(math.exp(v - m) for v in zz)), 2e-6 * (max(abs(v - m) for v in zz) + math.log(C) + 1)

        for w in range(S):
            want_ref[w], wb_ref[w] = s_of(z[w * (G + 1)], cls[w])
            for g in range(G):
                s, b = s_of(z[w * (G + 1) + 1 + g], cls[w])
                want[w, g] = want_ref[w] - s
                wb[w, g] = U * abs(want[w, g]) if score == 'logit' else wb_ref[w] + b
        sref, drop, bref, bdrop = K.ref_occlusion_drop(z, cls, S, G, score)
        assert np.allclose(sref, want_ref, rtol=1e-13, atol=1e-13) and np.allclose(drop, want, rtol=1e-13, atol=1e-13)
        assert np.allclose(bref, wb_ref, rtol=1e-13, atol=0) and np.allclose(bdrop, wb, rtol=1e-13, atol=0)


def test_seed_ref():
    rs = np.random.RandomState(6)
    B, C = 4, 3
    z = (rs.randn(B, C) * 8).astype(np.float32)
    z[0] = [0.5, 31.0, -0.25]                           # confident
    t = np.array([1, 0, 2, 1])
    d, bound = K.ref_seed(z, t, 'logit')
    assert np.array_equal(d, np.eye(C)[t]) and not bound.any()
    d, bound = K.ref_seed(z, t, 'logprob')
    for r in range(B):
        zz = [float(v) for v in z[r]]
        m = max(zz)
        e = [math.exp(v - m) for v in zz]
        for c in range(C):
            want = (1.0 if c == t[r] else 0.0) - e[c] / sum(e)
            if c == t[r]:                               # the literal form cancels on the confident row: compare as far as it holds
                assert abs(d[r, c] - want) <= 4e-16
            else:
                assert abs(d[r, c] - want) <= 1e-15 * abs(want)
        assert bound[r, 0] == 2e-6 * np.abs(d[r]).max()
    assert 0 < d[0, 1] < 1e-12 and abs(d[0].sum()) < 1e-25


def test_gradcam_refs():
    rs = np.random.RandomState(7)
    nw, F, N, P = 2, 3, 5, 2
    A, G = rs.randn(nw, F, _mp(N)).astype(np.float32), rs.randn(nw, F, _mp(N)).astype(np.float32)
    A[:, :, N:] = np.nan
    G[:, :, N:] = np.nan
    alpha, ab = K.ref_gradcam_weights(G, N)
    for r in range(nw):
        for f in range(F):
            want = sum(float(G[r, f, i]) for i in range(N)) / N
            assert abs(alpha[r, f] - want) <= 1e-15
            assert ab[r, f] >= np.spacing(np.float32(abs(want))) and ab[r, f] <= 1.001 * np.spacing(np.float32(abs(want)))
    a32 = alpha.astype(np.float32)
    order = np.array([3, -1, 0, 5, 1])                  # level vertices 1 and 3 write nothing: reference vertices 2, 4 unwritten
    for W in (a32, G):
        for relu in (False, True):
            for perm in (None, order):
                ldo = N * P + 3
                want, wb = np.full((nw, ldo), np.nan), np.zeros((nw, ldo))
                for r in range(nw):
                    for i in range(N):
                        j = perm[i] if perm is not None else i
                        if j < 0 or j >= N:
                            continue
                        terms = [float(W[r, f, i] if W.ndim == 3 else W[r, f]) * float(A[r, f, i]) for f in range(F)]
                        cam = sum(terms)
                        for q in range(P):
                            want[r, j * P + q] = max(cam, 0.0) if relu else cam
                            wb[r, j * P + q] = F * U * sum(abs(t) for t in terms)
                ref, bound = K.ref_gradcam_map(A, W, N, P, relu, perm, ldo)
                assert np.array_equal(np.isnan(ref), np.isnan(want))
                assert np.allclose(ref, want, rtol=1e-14, atol=1e-300, equal_nan=True) and np.allclose(bound, wb, rtol=1e-14, atol=0)
                if perm is not None:
                    assert np.isnan(ref[:, [4, 5, 8, 9]]).all() and int(np.isnan(ref[0, :N * P]).sum()) == 2 * P
