"""The two kinds of ``WindowSet`` share one core: a start-cut set and an event set staged over the same small series, the
event set's index tables spelling out the start-cut windows (``start + arange(C)``, ``fold = 1``), stand for the same array
bit for bit -- plain, with tables, and balanced by re-drawn (``sampling = 1``) and by synthetic (``sampling = 3``) windows out
of the same seed and groups.  CPU tensors and a stub owner with a vertex order of its own.  No GPU."""
import numpy as np
import pytest
import torch

from gcn_fmri_decoding_amd import decode, series

M, MP, C = 5, 32, 3
LENGTHS = [12, 9]
STARTS = [np.array([0, 9, 4, 4, 7]), np.array([6, 0, 3, 1])]
LABELS = np.array([0, 0, 1, 0, 2, 0, 1, 0, 0])                  # [6, 2, 1] windows per class: classes 1 and 2 are topped up
GROUPS = [4, 9]


class _Owner(object):
    """What a ``WindowSet`` asks of its model: sizes, a device, the internal vertex order and the tables in that order."""
    _M0, channel, device = M, C, torch.device('cpu')
    _order = np.array([3, 0, 4, 1, 2])                          # internal vertex j is the caller's vertex _order[j]
    _scale_tables = decode.Decode._scale_tables


def _sets():
    rs = np.random.RandomState(11)
    runs = [rs.randn(T, M).astype(np.float32) for T in LENGTHS]
    owner = _Owner()
    planes = torch.zeros((sum(LENGTHS), MP), dtype=torch.float32)
    planes[:, :M] = torch.as_tensor(np.concatenate(runs)[:, owner._order])
    index = [s[:, None] + np.arange(C)[None, :] for s in STARTS]
    ws = series.StartWindowSet(owner, planes, LENGTHS, STARTS, M, C)
    we = series.EventWindowSet(owner, planes, LENGTHS, index, M, C, 1)
    cut = np.stack([r[s:s + C].T for r, st in zip(runs, STARTS) for s in st])          # [S, M, C], the caller's order
    return ws, we, cut, rs.rand(M, C).astype(np.float32) + 0.5, rs.randn(M, C).astype(np.float32)


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


@pytest.mark.parametrize('tables', [False, True])
@pytest.mark.parametrize('sampling', [0, 1, 3])
def test_start_cut_and_event_sets_stand_for_the_same_array(sampling, tables):
    ws, we, cut, scale, shift = _sets()
    S = len(LABELS)
    for w in (ws, we):
        assert isinstance(w, series.WindowSet) and len(w) == S and w.shape == (S, M, C) and w.sources is None
        if tables:
            w.set_tables(scale, shift)
    want = (cut * scale[None]).astype(np.float32) + shift[None] if tables else cut
    assert np.array_equal(_bits(ws.materialise()), _bits(want)) and np.array_equal(_bits(we.materialise()), _bits(want))
    la, lb = (w.balance(LABELS, sampling, 5, GROUPS) for w in (ws, we))
    assert np.array_equal(la, lb) and la.dtype == lb.dtype
    if sampling:
        assert len(la) == 6 * 3 and np.bincount(la).tolist() == [6, 6, 6]
        for a, b in zip(ws.sources, we.sources):
            assert np.array_equal(a, b) and a.dtype == b.dtype
        src, cnt = ws.sources
        assert src.shape == (18, sampling) and (cnt[:S] == 1).all() and (cnt[S:] == sampling).all()
    else:
        assert ws.sources is None and we.sources is None and np.array_equal(la, LABELS)
    assert len(ws) == len(we) == len(la) and ws.shape == we.shape == (len(la), M, C)
    xa, xb = ws.materialise(), we.materialise()
    assert xa.dtype == np.float32 and xa.shape == ws.shape and np.array_equal(_bits(xa), _bits(xb))
    assert np.array_equal(_bits(xa[:S]), _bits(want))                                   # the originals stay in front, untouched
    for w in (ws, we):
        assert w.balance(None, 0) is None and len(w) == S and w.shape == (S, M, C) and w.sources is None
    assert np.array_equal(_bits(ws.materialise()), _bits(want)) and np.array_equal(_bits(we.materialise()), _bits(want))


def test_only_the_start_cut_set_can_be_displaced():
    ws, we, _, _, _ = _sets()
    assert we.jitter == 0
    with pytest.raises(ValueError, match='cannot be displaced'):
        we.jitter = 1
    with pytest.raises(ValueError, match='cannot be displaced'):
        we.set_rows(np.zeros(len(we), np.int64))
    ws.jitter, ws.jitter_rng = 1, np.random.RandomState(0)
    assert np.abs(ws.refill() - np.concatenate(STARTS)).max() == 1 and np.array_equal(we.refill(), we.starts)
