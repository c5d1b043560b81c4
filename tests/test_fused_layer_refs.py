"""The float64 references of tests/test_gpu_fused_layer_arms.py against literal nested-loop transcriptions of the header comment
of csrc/fused_small.hip on one tiny shape each, and the host-side figures that test relies on.  No GPU: this is what shows, on
any machine, that the vectorised references say what the header says."""
import numpy as np
import torch

import test_gpu_fused_layer_arms as T


def _tiny_operator():
    """Five vertices, non-symmetric, vertex 3 isolated (empty row and column): CSR with fp32 values."""
    rows = [[(1, 0.5), (4, -0.25)], [(0, 0.125), (2, 0.75), (4, 0.3)], [(1, -0.6)], [], [(0, 0.2), (2, 0.1)]]
    indptr, indices, data = [0], [], []
    for r in rows:
        for c, v in r:
            indices.append(c)
            data.append(v)
        indptr.append(len(indices))
    return np.array(indptr, np.int32), np.array(indices, np.int32), np.array(data, np.float32)


def _loop_matvec(indptr, indices, data, t, transposed=False):
    """(L t)[m] = sum over the entries e of row m, in CSR order, of val[e] * t[col[e]]; transposed: scattered instead."""
    M = len(indptr) - 1
    out = [0.0] * M
    for m in range(M):
        for e in range(indptr[m], indptr[m + 1]):
            if transposed:
                out[indices[e]] += float(data[e]) * t[m]
            else:
                out[m] += float(data[e]) * t[indices[e]]
    return out


def test_dense_operator_is_the_csr():
    indptr, indices, data = _tiny_operator()
    D = T.dense_operator(indptr, indices, data, 5).numpy()
    assert D.dtype == np.float64 and np.count_nonzero(D) == len(data)
    for m in range(5):
        for e in range(indptr[m], indptr[m + 1]):
            assert D[m, indices[e]] == float(data[e])          # the fp32 value, exactly
    assert not D[3].any() and not D[:, 3].any()


def test_forward_ref():
    indptr, indices, data = _tiny_operator()
    rs = np.random.RandomState(0)
    B, Fin, M, Fout = 2, 3, 5, 2
    D = T.dense_operator(indptr, indices, data, M)
    for K in (1, 2, 3, 5):
        x, W = rs.randn(B, Fin, M), rs.randn(Fin * K, Fout)
        for bias in (None, rs.randn(Fout), rs.randn(Fout, M)):
            for relu in (False, True):
                stack = np.zeros((K, B, Fin, M))
                y = np.zeros((B, Fout, M))
                for b in range(B):
                    for f in range(Fin):
                        t = [list(x[b, f])]
                        if K > 1:
                            t.append(_loop_matvec(indptr, indices, data, t[0]))
                        for k in range(2, K):
                            lt = _loop_matvec(indptr, indices, data, t[k - 1])
                            t.append([2 * lt[m] - t[k - 2][m] for m in range(M)])
                        stack[:, b, f] = t
                    for o in range(Fout):
                        for m in range(M):
                            s = 0.0
                            for f in range(Fin):
                                for k in range(K):
                                    s += W[f * K + k, o] * stack[k, b, f, m]
                            if bias is not None:
                                s += bias[o] if bias.ndim == 1 else bias[o, m]
                            y[b, o, m] = s
                act = np.maximum(y, 0.0) if relu else y
                gy, gact, gstack = T.ref_forward(D, torch.as_tensor(x), torch.as_tensor(W), K,
                                                 None if bias is None else torch.as_tensor(bias), relu)
                assert gy.dtype == torch.float64
                np.testing.assert_allclose(gstack.numpy(), stack, rtol=0, atol=1e-13)
                np.testing.assert_allclose(gy.numpy(), y, rtol=0, atol=1e-13)
                np.testing.assert_allclose(gact.numpy(), act, rtol=0, atol=1e-13)
                assert np.array_equal(gstack[0].numpy(), x)


def test_backward_ref():
    """The Clenshaw adjoint of the header, by loops; and as what it is: the transpose of the forward map (<dy, y(x)> = <dx, x>
    for the linear layer), on the non-symmetric operator."""
    indptr, indices, data = _tiny_operator()
    rs = np.random.RandomState(1)
    B, Fin, M, Fout = 2, 3, 5, 4
    D = T.dense_operator(indptr, indices, data, M)
    for K in (1, 2, 3, 4, 6):
        W, dy = rs.randn(Fin * K, Fout), rs.randn(B, Fout, M)
        for gate in (None, rs.rand(B, Fout, M) > 0.4):
            dyg = dy if gate is None else np.where(gate, dy, 0.0)
            dx = np.zeros((B, Fin, M))
            for b in range(B):
                for f in range(Fin):
                    G = [[sum(W[f * K + j, o] * dyg[b, o, m] for o in range(Fout)) for m in range(M)] for j in range(K)]
                    c = {K: [0.0] * M, K + 1: [0.0] * M}
                    for j in range(K - 1, 0, -1):                                          # c_j = G_j + 2 L^T c_{j+1} - c_{j+2}
                        lt = _loop_matvec(indptr, indices, data, c[j + 1], transposed=True)
                        c[j] = [G[j][m] + 2 * lt[m] - c[j + 2][m] for m in range(M)]
                    c.setdefault(1, [0.0] * M)
                    c.setdefault(2, [0.0] * M)
                    lt = _loop_matvec(indptr, indices, data, c[1], transposed=True)
                    dx[b, f] = [G[0][m] + lt[m] - c[2][m] for m in range(M)]             # dx = G_0 + L^T c_1 - c_2
            got = T.ref_backward(D, torch.as_tensor(dy), None if gate is None else torch.as_tensor(gate), torch.as_tensor(W), Fin, K)
            np.testing.assert_allclose(got.numpy(), dx, rtol=0, atol=1e-12)
            x = rs.randn(B, Fin, M)
            y = T.ref_forward(D, torch.as_tensor(x), torch.as_tensor(W), K)[0].numpy()
            assert abs((dyg * y).sum() - (dx * x).sum()) <= 1e-11 * np.abs(dyg * y).sum()
    # the operator is told from its transpose
    dx_t = T.ref_backward(D.T.contiguous(), torch.as_tensor(dy), None, torch.as_tensor(W), Fin, K).numpy()
    assert np.abs(dx_t - dx).max() > 1e-2 * np.abs(dx).max()


def test_mask_bits_ref():
    Mp = 32
    rs = np.random.RandomState(2)
    m = rs.randint(0, 16, (2, 3, Mp // 4)).astype(np.uint8)
    bits = T.mask_bits(torch.as_tensor(m), Mp).numpy()
    for b in range(2):
        for o in range(3):
            for v in range(Mp):
                assert bits[b, o, v] == bool((m[b, o, v // 4] >> (v & 3)) & 1)


def test_launch_geometry_ref():
    """fs_lds / the slot count of fs_launch by hand at the shapes the GPU test leans on (256 CUs)."""
    assert T.launch_geometry(12, 16, 3, 515, 256) == (67584, 512, 515)             # two workgroups per CU
    assert T.launch_geometry(12, 16, 10, 515, 256) == (96256, 256, 515)
    assert T.launch_geometry(12, 8, 16, 150, 256) == (96256, 256, 300)
    assert T.launch_geometry(8, 8, 16, 150, 256) == (86016, 256, 300)
    assert T.launch_geometry(8, 16, 31, 1, 256)[0] == 160 * 1024 and T.launch_geometry(8, 16, 32, 1, 256)[0] > 160 * 1024
    assert T.launch_geometry(12, 16, 26, 1, 256)[0] == 161792 and T.launch_geometry(12, 16, 27, 1, 256)[0] > 160 * 1024
    assert T.launch_geometry(8, 8, 3, 7, 255)[1] == 510                            # an even number of slots for half-windows


def test_host_side_figures_of_the_gpu_cases():
    """Longest rows of the graphs the GPU test names its kernels by, and that its table reaches all sixteen instantiations."""
    for (N, k) in T.SYNTHETIC:
        T.synthetic_checked(N, k)
    names = T.instantiation_names()
    assert len(names) == 16 and names == {'fused_layer_kernel<%d,%d,%s,%d>' % (nw, pl, adj, ml) for nw in (8, 12) for pl in (8, 16)
                                          for adj in ('false', 'true') for ml in (16, 20)}
    for M, k, ml in T.VERTICES:
        op = T.knn(M, k, isolated=(1, M // 2, M - 1))
        assert T.Operator.ml(op.len_fwd) == ml and op.len_fwd == op.len_adj
    for M in (200, 300):
        a, at = T.ring(M, False), T.ring(M, True)
        assert (a.len_fwd, a.len_adj, at.len_fwd, at.len_adj) == (5, 19, 19, 5)
        assert np.array_equal(a.dense().numpy().T, at.dense().numpy())
