"""Host companion of tests/test_gpu_staging_kernels.py: the case tables of tests/staging_kernel_cases.py reach every edge of the
staging and feature-mean kernels they name (asserted from the shapes alone), the references are what they claim to be, and the
guarded regions sit where the device module says.  No GPU."""
import numpy as np
import pytest

from gcn_fmri_decoding_amd import _lib
from gcn_fmri_decoding_amd._lib import plane_stride
from oracle import coarsening_ref

import guarded_buffers as gb
import staging_kernel_cases as K

TURN = 4 * 256                  # elements one turn of perm_data_kernel's gather loop takes
BLOCK = 64                      # output columns of one workgroup of the staging kernels


def shapes(entry):
    return [c.shape for c in K.staging(entry)]


def test_case_ids_are_unique_and_every_entry_occurs():
    ids = [c.id for table in (K.STAGING, K.OPTIMIZER, K.LOSS, K.SCALARS, K.XENT) for c in table]
    assert len(ids) == len(set(ids))
    assert K.entries_reached() == set(K.ENTRIES)
    for e in K.ENTRIES + ('chebgcn_adam_partials',):
        assert e in _lib.SIGNATURES, e


@pytest.mark.parametrize('entry', ['perm_data', 'to_plane', 'from_plane'])
def test_tile_kernels_reach_their_edges(entry):
    ss = shapes(entry)
    Fs, Ms = {s.F for s in ss}, {s.M for s in ss}
    assert set(K.F_SWEEP) <= Fs and set(K.M_SWEEP) <= Ms
    assert all(s.F <= K.F_MAX and (getattr(s, 'S', None) or s.B) <= 3 for s in ss)
    # the gather loop: three quarters of the workgroup on the clamp; exactly one turn; a second turn of at most 64 elements;
    # several whole turns and a tail; the last width the LDS check admits, the next one refused
    assert any(BLOCK * s.F <= TURN // 4 for s in ss)
    assert any(BLOCK * s.F == TURN for s in ss)
    assert any(0 < BLOCK * s.F % TURN <= 64 and BLOCK * s.F > TURN for s in ss)
    assert any(BLOCK * s.F > 2 * TURN and BLOCK * s.F % TURN for s in ss)
    assert any(s.F % 4 for s in ss) and any(s.F % 4 == 0 for s in ss)
    assert 65 * K.F_MAX * 4 <= 64 * 1024 < 65 * (K.F_MAX + 1) * 4 and K.F_MAX in Fs
    # the store guard: Mp no multiple of the block (columns of the last block beyond Mp), a block across [M, Mp), a block
    # that ends at M, one block only and more than two
    assert any(plane_stride(s.M) % BLOCK for s in ss)
    assert any(s.M // BLOCK == (plane_stride(s.M) - 1) // BLOCK and s.M % BLOCK and s.M > BLOCK for s in ss)
    assert any(s.M % BLOCK == 0 for s in ss) and any(s.M < BLOCK for s in ss) and any(s.M > 2 * BLOCK for s in ss)
    assert any(s.M == 1 for s in ss)
    for F in K.F_OF_M_SWEEP:
        assert {s.M for s in ss if s.F == F} >= set(K.M_SWEEP)


def test_perm_data_cases_reach_every_kind_of_permutation_and_sample():
    cases = K.staging('perm_data')
    kinds = {c.shape.kind for c in cases}
    assert kinds == {'fakes', 'subset', 'repeats', 'edge', 'identity'}
    for c in cases:
        s, perm = c.shape, c.built().inp['perm']
        assert s.S <= 3 and s.S_total <= 3
        if s.kind == 'identity':
            assert perm is None and s.M == s.N
            continue
        assert perm.dtype == np.int32 and perm.shape == (s.M,)
        if s.kind == 'fakes':
            assert s.M > s.N and sorted(perm.tolist()) == list(range(s.M))
        elif s.kind == 'subset':
            assert s.M <= s.N and len(set(perm.tolist())) == s.M and perm.min() >= 0 and perm.max() < s.N
        elif s.kind == 'repeats':
            assert len(set(perm.tolist())) < s.M and perm.min() >= 0 and perm.max() < s.N
        else:
            assert {s.N, s.N + 1, K.INT32_MAX, -1, K.INT32_MIN} <= set(perm.tolist())
            assert (perm < 0).any() and (perm >= s.N).any()
            inside = (perm >= 0) & (perm < s.N)
            # scattered: an outside entry with valid neighbours, in the first and last column and on both sides of a block boundary
            assert not inside[0] and not inside[s.M - 1] and not inside[BLOCK - 1] and not inside[BLOCK]
            assert any(not inside[i] and inside[i - 1] and inside[i + 1] for i in range(1, s.M - 1))
            assert inside.sum() > s.M // 2
    samples = [c.shape.sample for c in cases if c.shape.S_total == 3]
    assert None in samples and [2, 1, 0] in samples and [2, 0, 2] in samples and [1] in samples
    assert all(max(sm) < 3 and min(sm) >= 0 for sm in samples if sm is not None)        # sample stays the caller's duty


def test_perm_data_reference_is_the_oracles_where_both_are_defined():
    compared = 0
    for c in K.staging('perm_data'):
        b, s = c.built(), c.shape
        x, perm, sample = b.inp['x'], b.inp['perm'], b.inp['sample']
        assert b.ref.shape == (s.S, s.F, plane_stride(s.M)) and b.ref.dtype == np.float32
        assert not b.ref[:, :, s.M:].any()
        if not K.oracle_defined(perm, s.N):
            continue
        xs = x if sample is None else x[sample]
        want = coarsening_ref.perm_data_3d(xs, perm)                     # [S, M, F] float64
        assert np.array_equal(want.astype(np.float32).astype(np.float64), want)
        assert np.array_equal(gb.bits(K.from_plane_ref(b.ref, s.M)), gb.bits(want.astype(np.float32))), c.id
        compared += 1
    assert compared >= 10
    # the header's rule where the oracle is not defined: every column of an outside entry is zero, the others are copies
    c = next(c for c in K.staging('perm_data') if c.shape.kind == 'edge')
    b, s = c.built(), c.shape
    perm = b.inp['perm'].astype(np.int64)
    for i in range(s.M):
        col = b.ref[:, :, i]
        if 0 <= perm[i] < s.N:
            assert np.array_equal(gb.bits(col), gb.bits(b.inp['x'][:, perm[i], :]))
        else:
            assert not col.any()


def test_plane_references_round_trip():
    for c in K.staging('to_plane'):
        b = c.built()
        assert np.array_equal(gb.bits(K.from_plane_ref(b.ref, c.shape.M)), gb.bits(b.inp['x']))
        assert np.array_equal(gb.bits(b.ref), gb.bits(K.perm_data_ref(b.inp['x'], None, None, c.shape.M)))
    for c in K.staging('from_plane'):
        b = c.built()
        xp = b.inp['xp']
        assert np.isnan(xp[:, :, c.shape.M:]).all() and not np.isnan(xp[:, :, :c.shape.M]).any()
        assert np.array_equal(gb.bits(K.from_plane_ref(xp, c.shape.M)), gb.bits(b.ref)) and not np.isnan(b.ref).any()


def test_feature_mean_cases_and_references():
    fwd, bwd = K.staging('feature_mean_fwd'), K.staging('feature_mean_bwd')
    for cases in (fwd, bwd):
        ss = [c.shape for c in cases]
        assert {s.M for s in ss if s.F == K.MEAN_F_AT_M} >= set(K.MEAN_M_SWEEP)
        assert {s.F for s in ss if s.M == K.MEAN_M_AT_F} >= set(K.MEAN_F_SWEEP)
        # eight planes per turn: no tail, a tail of one and of seven, F below one turn, several turns; the 256-vertex workgroup:
        # one short of it, exactly it, one more
        assert any(s.F % 8 == 0 for s in ss) and any(s.F % 8 == 1 and s.F > 8 for s in ss) and any(s.F % 8 == 7 for s in ss)
        assert any(s.F % 8 and s.F > 16 for s in ss) and any(s.F == 1 for s in ss)
        assert {255, 256, 257} <= {s.M for s in ss} and all(s.B <= 3 for s in ss)
    differs = 0
    for c in fwd:
        b, s = c.built(), c.shape
        x = b.inp['x']
        assert np.isnan(x[:, :, s.M:]).all() and not np.isnan(x[:, :, :s.M]).any()
        assert b.ref.dtype == np.float32 and b.ref.shape == b.ref64.shape == b.bound.shape == (s.B, s.M)
        err = np.abs(b.ref.astype(np.float64) - b.ref64)
        assert (err <= b.bound).all(), '%s: the float32 restatement is %.3g of the bound from the float64 mean' % (c.id, (err / b.bound).max())
        # the bound is tight enough for one duplicated or dropped plane: that moves the mean by about 1 / F of itself
        assert (b.bound < 0.01 * np.abs(b.ref64) / s.F).all()
        if s.F >= 7:
            # otherwise the exact assertion would prove nothing about the order of the additions
            assert (b.ref.astype(np.float64) != b.ref64).any(), c.id
            differs += 1
        if s.F == 1:
            assert np.array_equal(gb.bits(b.ref), gb.bits(x[:, 0, :s.M]))
    assert differs >= 8
    for c in bwd:
        b, s = c.built(), c.shape
        assert b.ref.shape == (s.B, s.F, plane_stride(s.M)) and not b.ref[:, :, s.M:].any()
        want = b.inp['dy'].astype(np.float64) / s.F
        assert (np.abs(b.ref[:, :, :s.M] - want[:, None, :]) <= K.U * np.abs(want)[:, None, :]).all()
        assert (b.ref == b.ref[:, :1, :]).all()


def test_addition_order_shows_in_the_float32_restatement():
    """Descending f gives other bits somewhere: the exact comparison pins the order, not only the set of planes."""
    c = next(c for c in K.staging('feature_mean_fwd') if c.shape.F == 65)
    x, M = c.built().inp['x'], c.shape.M
    assert (K.feature_mean_ref32(x[:, ::-1], M) != c.built().ref).any()


def test_optimizer_tables():
    assert K.ADAM_N == (1, 255, 256, 257, 4096 * 256 + 1)
    for c in K.OPTIMIZER:
        assert c.n in K.ADAM_N and (c.n_reg is None or 0 <= c.n_reg <= c.n)
    for entry in ('chebgcn_adam_step', 'chebgcn_adam_step_dev', 'chebgcn_adam_step_sq'):
        assert {c.n for c in K.OPTIMIZER if c.entry == entry} == set(K.ADAM_N)
    for entry in ('chebgcn_adam_step_sq_all', 'chebgcn_nadam_step_sq_all'):
        for n in K.ADAM_N:
            assert {c.n_reg for c in K.OPTIMIZER if c.entry == entry and c.n == n} == {0, n // 3, n}
    assert {True, False} == {c.lr_dev for c in K.OPTIMIZER if c.sq}
    L = _lib.lib()
    for n in K.ADAM_N + (0, 4096 * 256, 4096 * 256 - 1):
        assert L.chebgcn_adam_partials(n) == K.adam_partials(n)
    # the largest case is the only one beyond the cap on the workgroups: its last partial is the 4096th
    assert K.adam_partials(max(K.ADAM_N)) == 4096 and (max(K.ADAM_N) + 255) // 256 == 4097
    assert 4 * 4 * max(K.ADAM_N) < 17 << 20
    assert {(c.nparts, c.loss_out, c.corr_dev) for c in K.LOSS} == {(n, lo, cd) for n in (0, 1, 1025, 4096) for lo in (False, True)
                                                                  for cd in (False, True)}
    assert {(c.B, c.C) for c in K.XENT} == {(1, 2), (257, 22), (33, 45)}
    for c in K.XENT:
        logits, labels = K.xent_inputs(c)
        assert labels.dtype == (np.int64 if c.int64 else np.int32) and logits.shape == (c.B, c.C)
        outside = (labels < 0) | (labels >= c.C)
        assert outside.sum() == (1 if c.bad else 0)
        if c.bad and c.int64:
            assert 0 <= int(labels[outside][0]) & 0xFFFFFFFF < c.C        # a kernel that truncated the label would find it valid


@pytest.mark.parametrize('align', [4, 8])
def test_guarded_regions_sit_at_the_weakest_alignment(align):
    for base in (0, 4, 8, 12, 16, 4096, 4100, 1 << 20, (1 << 20) + 24):
        for nbytes in (0, 4, 8, 4 * 4096, 4 * (4096 * 256 + 1)):
            off, whole = gb.layout(base, nbytes, align)
            a = base + off
            assert a % align == 0 and a % (2 * align) != 0
            assert off >= gb.GUARD_BYTES and whole - off - nbytes >= gb.GUARD_BYTES
    assert gb.fill_value(gb.FILL_A, 'float32') != gb.fill_value(gb.FILL_A, 'float32')       # NaN
    assert np.isfinite(gb.fill_value(gb.FILL_B, 'float32')) and gb.fill_value(gb.FILL_B, 'float32') > 1e15
