"""The three Shapley kernels (csrc/shapley.hip) BY NAME, on plain tensors, every element against NumPy, with the plumbing of
tests/test_gpu_attribution_kernels.py (sentinel-filled outputs inside sentinel margins, kernels named through
``chebgcn_last_dispatch()``, every launch twice).  Needs an MI355X: ``-m gpu``.

* shapley_rows only moves values: bit for bit against ``ref_shapley_rows``, a NumPy restatement of the header's contract.
* shapley_score: 'logit' is a copy (bit for bit); 'logprob' is the arithmetic of occlusion_score and held to its bound,
  2e-6 (max_k |z_k - max z| + log C + 1).
* shapley_reduce: float64 differences of float32 scores (exact: both within a few binades), added in float64 (2^-53
  relative per addition, far below a float32 ulp), one float64 division, one rounding to float32: within 1 ulp of float32 of
  the float64 formula evaluated on the table the GPU holds."""
import numpy as np
import pytest
import torch

from conftest import record_measured
from test_gpu_attribution_kernels import (Guarded, L, _bits, _named, _ok, _p, _refused, _s, _same_bits, _to, _within, dev,  # noqa: F401
                                          plane_stride, ref_class_score, ref_gather)

pytestmark = pytest.mark.gpu


def ref_shapley_rows(x, perm, gid, rank, x0, r0, R, M):
    """Rows r0 .. r0 + R of a Shapley run as planes [R, F, Mp] in x's dtype: row r is window r // (P (G + 1)), permutation
    (r // (G + 1)) % P, prefix j = r % (G + 1): the window's value where the position has no group or its group's rank in the
    permutation is below j, else the baseline (0 without one); 0 on the pad and past S P (G + 1)."""
    x = np.asarray(x)
    S, N, F = x.shape
    P, G = rank.shape
    Mp = plane_stride(M)
    r = r0 + np.arange(R, dtype=np.int64)
    w, p, j = r // (P * (G + 1)), (r // (G + 1)) % P, r % (G + 1)
    X = ref_gather(np.concatenate([x, np.zeros((1, N, F), x.dtype)]), perm, M)         # window S: the zero rows
    B0 = ref_gather(np.asarray(x0, x.dtype), perm, M) if x0 is not None else np.zeros((F, Mp), x.dtype)
    gp = np.full(Mp, -1, np.int64)
    gp[:M] = np.asarray(gid)
    pos = np.where(gp[None, :] >= 0, np.asarray(rank, np.int64)[p][:, np.maximum(gp, 0)], -1)      # [R, Mp]
    own = (pos < j[:, None]) | (w >= S)[:, None]
    return np.where(own[:, None, :], X[np.minimum(w, S)], B0[None])


def _rank_of(perms):
    rank = np.empty_like(perms)
    np.put_along_axis(rank, perms, np.arange(perms.shape[1], dtype=perms.dtype)[None, :], axis=1)
    return rank


def _perms(rs, P, G):
    return np.stack([rs.permutation(G) for _ in range(P)]).astype(np.int32)


@pytest.mark.parametrize('F', [1, 15, 125])
@pytest.mark.parametrize('M', [63, 64, 65, 130])
def test_shapley_rows(dev, L, M, F):
    """The tile edges (M = 63, 64, 65: one tile and one position into the second; 130: three tiles, the pad [130, 160)), the
    channel edges (F = 125 is the limit of chebgcn_shapley_supported), G + 1 = 2, 3, 8 against the 16-row chunk of a workgroup
    (eight permutations per workgroup; chunks that straddle permutations and windows), P = 1 and 3, groups with and without
    positions outside the game, a scattered vertex map with fake positions, with and without a baseline.  Passes: the whole
    run and five rows behind it; from row 1 into the next window; from row 5 for 30 rows (at G = 7, P = 3 it ends inside
    permutation 1 of window 1); the last row of the run and 19 rows behind it."""
    from gcn_fmri_decoding_amd import ops
    rs = np.random.RandomState(1000 * M + F)
    S, N = 3, M - 3
    x = rs.randn(S, N, F).astype(np.float32)
    x0 = rs.randn(N, F).astype(np.float32)
    perm = rs.permutation(M).astype(np.int32)           # entries >= N: fake positions
    xd, bd, pd = _to(x, dev), _to(x0, dev), _to(perm, dev)
    for G in (1, 2, 7):
        for holes in (False, True):
            gid = rs.randint(-1 if holes else 0, G, M).astype(np.int32)
            gid[rs.permutation(M)[:G]] = np.arange(G)
            gd = _to(gid, dev)
            for P in (1, 3):
                rank = _rank_of(_perms(rs, P, G))
                rd = _to(rank, dev)
                per = P * (G + 1)
                total = S * per
                for r0, R in [(0, total + 5), (1, per + (G + 1) // 2), (5, 30), (total - 1, 20)]:
                    out = Guarded((R, F, plane_stride(M)), torch.float32, dev)
                    for base, based in ((None, None), (x0, bd)):
                        out.refill()
                        _ok(L.chebgcn_shapley_rows(_p(xd), _p(pd), _p(gd), _p(rd), _p(based), _p(out.t), r0, R, S, P, G, N, M, F,
                                                   _s()), 'shapley_rows')
                        _named('shapley_rows_kernel')
                        got = out.t.cpu().numpy()
                        assert out.margins_intact()
                        ref = ref_shapley_rows(x, perm, gid, rank, base, r0, R, M)
                        assert _same_bits(got, ref), 'rows G=%d holes=%s P=%d r0=%d R=%d baseline=%s: %d elements differ' % (
                            G, holes, P, r0, R, base is not None, int((_bits(got) != _bits(ref)).sum()))
                        assert not got[:, :, M:].any() and not got[max(0, total - r0):].any()
                        again = ops.shapley_rows(xd, pd, gd, rd, based, r0, R, M)
                        _named('shapley_rows_kernel')
                        assert torch.equal(again, out.t)


def test_shapley_rows_prefixes_are_what_the_definition_says(dev):
    """Against the words of the definition, not the restatement above: identity order, one window, G = 7, P = 3: row 0 of a
    permutation is the baseline (but for group -1), row G the window itself, and row j + 1 differs from row j on exactly the
    vertices of the permutation's group j."""
    from gcn_fmri_decoding_amd import ops
    rs = np.random.RandomState(5)
    M, F, G, P = 70, 2, 7, 3
    x, x0 = rs.randn(1, M, F).astype(np.float32), rs.randn(M, F).astype(np.float32)
    gid = rs.randint(-1, G, M).astype(np.int32)
    gid[:G] = np.arange(G)
    perms = _perms(rs, P, G)
    rows = ops.shapley_rows(_to(x, dev), None, _to(gid, dev), _to(_rank_of(perms), dev), _to(x0, dev), 0, P * (G + 1), M)
    rows = rows.cpu().numpy().reshape(P, G + 1, F, plane_stride(M))[..., :M].transpose(0, 1, 3, 2)      # [P, G + 1, M, F]
    for p in range(P):
        start = np.where((gid < 0)[:, None], x[0], x0)
        assert np.array_equal(rows[p, 0], start) and np.array_equal(rows[p, G], x[0])
        for j in range(G):
            changed = (rows[p, j + 1] != rows[p, j]).any(axis=1)
            assert np.array_equal(changed, gid == perms[p, j])


def test_shapley_rows_refusals(dev, L):
    """One channel more than chebgcn_shapley_supported admits: the status code, the reason, nothing launched."""
    x, gid = torch.zeros((1, 64, 126), device=dev), torch.zeros(64, dtype=torch.int32, device=dev)
    rank = torch.zeros((1, 1), dtype=torch.int32, device=dev)
    out = Guarded((8, 126, 64), torch.float32, dev)
    assert L.chebgcn_shapley_supported(125) == 1 and L.chebgcn_shapley_supported(126) == 0
    _refused(L, L.chebgcn_shapley_rows(_p(x), None, _p(gid), _p(rank), None, _p(out.t), 0, 8, 1, 1, 1, 64, 64, 126, _s()),
             'too large')
    _refused(L, L.chebgcn_shapley_rows(_p(x), None, _p(gid), None, None, _p(out.t), 0, 8, 1, 1, 1, 64, 64, 3, _s()), 'NULL')
    _refused(L, L.chebgcn_shapley_rows(_p(x), None, _p(gid), _p(rank), None, _p(out.t), 0, 8, 1, 1, 1, 60, 64, 3, _s()),
             'identity')
    torch.cuda.synchronize()
    assert bool(torch.isnan(out.full).all())


@pytest.mark.parametrize('score', ['logit', 'logprob'])
def test_shapley_score_and_reduce(dev, score):
    """S = 3, P = 5, G = 7, C = 4, random logits: the score table filled in one pass, in passes of 64 and of 13 rows (the last
    one running 7 rows past the table: nothing behind it is written), then reduced; every launch twice."""
    from gcn_fmri_decoding_amd import ops
    rs = np.random.RandomState(17)
    S, P, G, C = 3, 5, 7, 4
    total = S * P * (G + 1)
    z = (rs.randn(total, C) * 4).astype(np.float32)
    cls = rs.randint(0, C, S).astype(np.int64)
    perms = _perms(rs, P, G)
    rank = _rank_of(perms)
    cd, rd = _to(cls, dev), _to(rank, dev)
    tables, phis = [], []
    for cut in (total, 64, 13, total):
        npass = (total + cut - 1) // cut
        zp = np.full((npass * cut, C), np.nan, np.float32)
        zp[:total] = z
        zd = _to(zp, dev)
        table, phi = Guarded((S, P, G + 1), torch.float32, dev), Guarded((S, G), torch.float32, dev)
        for k in range(npass):
            ops.shapley_score(zd[k * cut:(k + 1) * cut], k * cut, cd, score, table.t)
            _named('shapley_score_kernel<%s>' % score)
        ops.shapley_reduce(table.t, rd, phi.t)
        _named('shapley_reduce_kernel')
        assert table.margins_intact() and phi.margins_intact()
        tables.append(table.t.cpu().numpy())
        phis.append(phi.t.cpu().numpy())
    for t, f in zip(tables[1:], phis[1:]):
        assert _same_bits(t, tables[0]) and _same_bits(f, phis[0])
    sref, bound = ref_class_score(z, np.repeat(cls, P * (G + 1)), score)
    r1 = _within(tables[0].reshape(-1), sref, bound, 'score table')
    if score == 'logit':
        assert _same_bits(tables[0].reshape(-1), z[np.arange(total), np.repeat(cls, P * (G + 1))])
    t64 = tables[0].astype(np.float64)
    want = np.zeros((S, G))
    for p in range(P):                                  # p ascending, as the kernel adds
        want[:, perms[p]] += t64[:, p, 1:] - t64[:, p, :-1]
    want /= P
    ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    r2 = _within(phis[0], want, ulp, 'phi')
    # efficiency in the table: a window's row of phi sums to the mean of (last - first) over the permutations
    tele = (t64[:, :, -1] - t64[:, :, 0]).mean(axis=1)
    assert np.abs(phis[0].astype(np.float64).sum(axis=1) - tele).max() <= G * ulp.max()
    record_measured('shapley_score_reduce[%s]' % score, score_ratio_to_bound=r1, phi_ratio_to_ulp=r2)
    # a class outside [0, C): that window's scores and phi are NaN, the others unchanged
    bad = cls.copy()
    bad[1] = C
    table, phi = Guarded((S, P, G + 1), torch.float32, dev), Guarded((S, G), torch.float32, dev)
    ops.shapley_score(_to(z, dev), 0, _to(bad, dev), score, table.t)
    ops.shapley_reduce(table.t, rd, phi.t)
    tb, pb = table.t.cpu().numpy(), phi.t.cpu().numpy()
    assert np.isnan(tb[1]).all() and np.isnan(pb[1]).all()
    assert _same_bits(tb[[0, 2]], tables[0][[0, 2]]) and _same_bits(pb[[0, 2]], phis[0][[0, 2]])
