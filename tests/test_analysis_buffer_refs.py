"""The host side of tests/test_gpu_analysis_buffers.py, on a machine without a GPU (the library loads there and its queries are
host functions): (1) every analysis entry point of include/chebgcn.h that takes a non-const pointer has a case or a listed
exclusion; (2) every arm a case claims is one the geometry queries say its shape reaches; (3) every workspace query is positive
where a case uses a workspace and equals the case's own restatement of the formula the header documents -- where the header
gives NO formula the case says so (``ws_formula`` None) and the equality is skipped: today that is chebgcn_window_stats_workspace
(its count table has a lead the header does not state), chebgcn_knn_workspace and chebgcn_cheb_filter_workspace where noted in
their cases; (4) every case's host reference runs and is finite on the region it defines; (5) the guarded regions' layout and
the poison pairs are what guarded_buffers.py says.  No GPU."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT

import guarded_buffers as gb
import test_gpu_analysis_buffers as T
from test_abi_and_host import declared_symbols

# the sections of include/chebgcn.h the issue calls the analysis side: from the windows of scans to the SVM searchlight
FIRST_SECTION = '/* ---- training on scans'
END_SECTION = '/* ---- vertex order for the ordered recurrence kernels'

# entries with a non-const pointer that have no case here, each with its reason
EXCLUDED = {
    'chebgcn_fc_fwd_dropout': 'a head entry: guarded outputs and NaN poison in tests/test_gpu_uncertainty_kernels.py',
    'chebgcn_mc_reduce': 'guarded outputs and NaN poison in tests/test_gpu_uncertainty_kernels.py',
}
EXCLUDED.update(getattr(T, 'NOT_COVERED', {}))


def analysis_prototypes():
    """name -> parameter list (text) of every prototype declared in the analysis sections."""
    text = open(os.path.join(ROOT, 'include', 'chebgcn.h')).read()
    text = text[text.index(FIRST_SECTION):text.index(END_SECTION)]
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r'\b(chebgcn_[a-z0-9_]+)\s*\(([^;{}]*)\)\s*;', text)}


def writes_through_a_pointer(params):
    return any('*' in p and 'const' not in p for p in params.split(','))


def test_every_analysis_entry_with_an_output_pointer_has_a_case_or_a_stated_exclusion():
    protos = analysis_prototypes()
    assert set(protos) <= set(declared_symbols()) and len(protos) >= 40, sorted(protos)
    need = {n for n, p in protos.items() if writes_through_a_pointer(p)}
    assert 'chebgcn_window_drop' in need and 'chebgcn_searchlight_score' in need and 'chebgcn_knn_workspace' not in need
    covered = {e for c in T.CASES for e in c.entries}
    assert covered <= need, 'a case names an entry that is not an analysis entry with an output pointer: %s' % sorted(covered - need)
    assert not covered & set(EXCLUDED), sorted(covered & set(EXCLUDED))
    assert set(EXCLUDED) <= need, sorted(set(EXCLUDED) - need)
    missing = need - covered - set(EXCLUDED)
    assert not missing, 'no case in tests/test_gpu_analysis_buffers.py and no listed exclusion for: %s' % sorted(missing)
    assert all(isinstance(r, str) and len(r) > 20 for r in EXCLUDED.values())
    assert len({c.id for c in T.CASES}) == len(T.CASES)


@pytest.mark.parametrize('c', T.CASES, ids=[c.id for c in T.CASES])
def test_case_on_the_host(c):
    b = c.built()
    # (2) arms
    assert b.arms, c.id
    for claim, reached in b.arms:
        assert reached, '%s claims "%s", which its shape does not reach' % (c.id, claim)
    # (3) workspaces: exact bytes, positive where used, the header's formula where it gives one
    assert set(b.ws_formula) == set(b.ws)
    for name, n in b.ws.items():
        assert isinstance(n, int) and n >= 0
        f = b.ws_formula[name]
        if f is not None:
            assert n == f, '%s: workspace %s is %d bytes by the query, %d by the documented formula' % (c.id, name, n, f)
    # queries whose bytes the case lays out itself inside one output region (a plus yy of glm_workspace)
    for name, (n, f) in getattr(b, 'ws_checked', {}).items():
        assert n == f > 0, '%s: chebgcn_%s says %d bytes, the documented layout %d' % (c.id, name, n, f)
    # outputs: shapes, kinds and alignments are consistent; an accumulated-into output has a non-zero base
    for s in b.outs:
        assert s.kind.shape == s.shape and s.align in (1, 4, 8, 16) and set(np.unique(s.kind)) <= {0, 1, 2, 3}
        assert (s.accum is None) == (s.base is None) and s.base != 0
    # (4) the reference runs and is finite where it is defined
    ref = b.reference(b.inp)
    assert ref
    for name, r in ref.items():
        r = np.asarray(r)
        if r.dtype.kind == 'f':
            assert np.isfinite(r[~np.isnan(r)]).all() and (~np.isnan(r)).any(), (c.id, name)
    # inputs never read as data are NaN: the pad of every staged series, table and pattern matrix among the inputs
    for name, v in b.inp.items():
        if v is not None and name in ('planes', 'scale', 'shift', 'Xt', 'x') and v.dtype == np.float32 and v.ndim == 2 \
                and v.shape[1] % 32 == 0 and c.id != 'parcel_expand':
            assert np.isnan(v[:, -1]).all(), '%s: the pad of %s is not NaN' % (c.id, name)


def test_workspace_queries_are_zero_on_bad_shapes():
    L = T.lib()
    assert L.chebgcn_window_stats_workspace(0, 33, 3) == 0 and L.chebgcn_window_stats_indexed_workspace(0, 33, 3) == 0


def test_guarded_layout_and_poison_pairs():
    assert gb.GUARD_BYTES >= 4096 and gb.FILL_A == 0xFF and gb.FILL_B == 0x5A and 0 not in (gb.FILL_A, gb.FILL_B, gb.GUARD_BYTE)
    assert np.isnan(gb.fill_value(gb.FILL_A, 'float32')) and np.isnan(gb.fill_value(gb.FILL_A, 'float64'))
    assert gb.fill_value(gb.FILL_A, 'int32') == -1 and gb.fill_value(gb.FILL_A, 'uint8') == 255
    for dt in ('float32', 'float64'):
        v = gb.fill_value(gb.FILL_B, dt)
        assert np.isfinite(v) and v > 1e15
    assert gb.fill_value(gb.FILL_B, 'int32') == 0x5A5A5A5A > 10 ** 9
    assert gb.filled(gb.FILL_B, 'float64', (2, 3)).shape == (2, 3)
    for base in (0, 256, 512 + 4, 1000003):
        for align in (1, 4, 8, 16):
            for n in (0, 1, 4096 + 12):
                off, total = gb.layout(base, n, align)
                a = base + off
                assert off >= gb.GUARD_BYTES and total - off - n >= gb.GUARD_BYTES and a % align == 0
                assert align == 1 or a % (2 * align) == align
    # bits(): NaN equals the same NaN, -0.0 differs from 0.0
    assert (gb.bits(np.array([np.nan, -0.0], np.float32)) == gb.bits(np.array([np.nan, 0.0], np.float32))).tolist() == [True, False]
