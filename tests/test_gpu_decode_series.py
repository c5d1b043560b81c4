"""decode_series on the MI355X.  (1) chebgcn_contract_fwd_windows, every arm by name: bit for bit against chebgcn_contract_fwd on
the gathered stack (overlapping, repeated, unsorted starts) and on the very same memory (non-overlapping), and against float64
within the 1e-5 of the tensor's scale tests/test_gpu_dispatch.py holds contract_fwd to.  (2) cgcnn.decode_series end to end on
the networks of tests/test_gpu_saliency.py against the float64 RefNet on host-cut windows, both paths; strides, explicit
starts, lists of runs, chunking, scale / shift, batch sizes, reruns; what the shared path launches; the model's state;
checkpoints; finetuning_cgcnn."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import record_measured
from gcn_fmri_decoding_amd import _lib, decode, models_gcn, ops
from test_decode_host import host_windows, reference_logits
from test_gpu_saliency import BS, DEV, NETS, REL, WIDE_REL, _laplacians, _model, _reference, _same, _state

pytestmark = pytest.mark.gpu
KREL = 1e-5                 # the kernel against float64: what tests/test_gpu_dispatch.py holds contract_fwd to


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


RING, RINGP, SPLITK, PLAIN = ('contract_fwd_windows_ring_kernel', 'contract_fwd_windows_ring_kernel<pool>',
                              'contract_fwd_windows_splitk_kernel', 'contract_fwd_windows_kernel<1>')
MAX, AVG = 0, 1
NONE, FILTER, VERTEX = 0, 1, 2
# (B, M, C, K, Fout, pool, pool_kind, bias_kind, arm).  256 CUs: a launch is small while ceil(M / 512) * B < 512; the ring kernel
# takes C*K up to 352 rows (padded to 16) and, with a per-filter bias, Fout >= 4.
KERNEL_CASES = [
    # small launches: split-K, every pool
    (7, 360, 15, 5, 32, 1, MAX, VERTEX, SPLITK), (7, 360, 3, 4, 16, 2, MAX, FILTER, SPLITK), (5, 1000, 2, 3, 5, 4, AVG, VERTEX, SPLITK),
    (3, 100, 1, 1, 1, 1, MAX, FILTER, SPLITK), (13, 204, 3, 2, 5, 4, MAX, VERTEX, SPLITK), (13, 204, 2, 2, 16, 2, AVG, FILTER, SPLITK),
    (170, 1100, 3, 3, 16, 1, MAX, VERTEX, SPLITK),                    # 3 * 170 = 510 < 512: the last small launch at this plane size
    (511, 500, 15, 1, 32, 1, MAX, FILTER, SPLITK), (127, 2044, 2, 4, 5, 2, MAX, NONE, SPLITK),
    # big launches, pool 1: the ring kernel
    (171, 1100, 3, 3, 16, 1, MAX, VERTEX, RING),                      # 3 * 171 = 513: the first big one
    (513, 500, 15, 5, 32, 1, MAX, FILTER, RING), (171, 1100, 1, 1, 1, 1, MAX, VERTEX, RING), (129, 2044, 2, 2, 5, 1, MAX, FILTER, RING),
    (257, 520, 15, 23, 32, 1, MAX, VERTEX, RING),                     # 345 rows -> 352: the last ring shape
    (171, 1100, 3, 4, 4, 1, MAX, FILTER, RING), (173, 1100, 2, 3, 16, 1, AVG, NONE, RING),
    # big launches with pooling
    (171, 1100, 3, 3, 16, 2, MAX, VERTEX, RINGP), (171, 1100, 15, 2, 32, 4, MAX, FILTER, RINGP), (171, 1100, 2, 4, 5, 2, AVG, VERTEX, RINGP),
    (171, 1100, 3, 3, 16, 4, AVG, FILTER, RINGP), (129, 2044, 1, 2, 1, 4, MAX, VERTEX, RINGP),
    # big launches beyond the ring kernel's shapes
    (257, 520, 15, 24, 32, 1, MAX, VERTEX, PLAIN),                    # 360 rows -> 368 > 361
    (257, 520, 15, 24, 16, 2, AVG, FILTER, PLAIN), (171, 1100, 3, 2, 1, 1, MAX, FILTER, PLAIN), (171, 1100, 2, 3, 3, 4, MAX, FILTER, PLAIN),
]


def _pool64(y, pool, kind):
    if pool == 1:
        return y
    B, F, M = y.shape
    yr = y.reshape(B, F, M // pool, pool)
    return yr.max(dim=3).values if kind == MAX else yr.mean(dim=3)


@pytest.mark.parametrize('case', KERNEL_CASES, ids=lambda c: 'B%d-M%d-C%d-K%d-F%d-p%d%s-b%d-%s' % (c[:6] + ('max' if c[6] == MAX else 'avg', c[7], c[8])))
def test_windows_kernel_arm_bit_identical_and_vs_float64(case):
    assert torch.cuda.get_device_properties(0).multi_processor_count == 256, 'the dispatch arms asserted here assume 256 CUs'
    lib = _lib.lib()
    B, M, C, K, Fout, pool, pool_kind, bias_kind, arm = case
    assert lib.chebgcn_contract_fwd_windows_supported(B, M, C, K, Fout, pool) == 1
    Mp, Mo = ops.plane_stride(M), M // pool
    Mpo = ops.plane_stride(Mo)
    gen = torch.Generator(device=DEV)
    gen.manual_seed(B * 7919 + M * 31 + C * 7 + K)
    T = C + 37
    stack = torch.randn((K, T, Mp), generator=gen, device=DEV)
    stack[..., M:] = float('nan')                                     # the pad of a plane is never read as data
    starts = torch.randint(0, T - C + 1, (B,), generator=gen, device=DEV, dtype=torch.int32)      # overlapping, repeated, unsorted
    starts[0], starts[B // 2], starts[B - 1] = T - C, 0, T - C
    W = torch.randn((C * K, Fout), generator=gen, device=DEV) * (0.5 / np.sqrt(C * K))
    bias = None
    if bias_kind == VERTEX:
        bias = torch.zeros((Fout, Mp), device=DEV)
        bias[:, :M] = torch.randn((Fout, M), generator=gen, device=DEV) * 0.3
    elif bias_kind == FILTER:
        bias = torch.randn((Fout,), generator=gen, device=DEV) * 0.3
    st = stream()

    def run_windows(stk, Tn, tab, argmax):
        out = torch.full((B, Fout, Mpo), float('nan'), device=DEV)
        _lib.check(lib.chebgcn_contract_fwd_windows(P(stk), Tn, P(tab), P(W), P(bias), bias_kind, P(out), P(argmax), B, M, C, K, Fout,
                                                    pool, pool_kind, 1, st), 'contract_fwd_windows')
        assert _lib.last_dispatch() == arm, _lib.last_dispatch()
        return out

    def run_plain(stk, argmax):
        out = torch.full((B, Fout, Mpo), float('nan'), device=DEV)
        _lib.check(lib.chebgcn_contract_fwd(P(stk), P(W), P(bias), bias_kind, P(out), P(argmax), B, M, C, K, Fout, pool, pool_kind, 1,
                                            st), 'contract_fwd')
        assert _lib.last_dispatch() == arm.replace('_windows', ''), _lib.last_dispatch()
        return out
    nside = (Mp // 4) if pool == 1 else Mpo
    side = [torch.zeros((B, Fout, nside), dtype=torch.uint8, device=DEV) for _ in range(4)]
    live = (M // 4) if pool == 1 else Mo
    # overlapping windows against the gathered stack [K][B][C][Mp]
    idx = (starts.long()[:, None] + torch.arange(C, device=DEV)[None, :]).reshape(-1)
    gathered = stack[:, idx].reshape(K, B, C, Mp).contiguous()
    got = run_windows(stack, T, starts, side[0])
    want = run_plain(gathered, side[1])
    assert torch.equal(got[..., :Mo], want[..., :Mo]), 'windows and gathered stack differ'
    assert torch.equal(side[0][..., :live], side[1][..., :live]), 'argmax / ReLU mask differ'
    # non-overlapping windows: the two entries read the very same memory
    T2 = B * C
    stack2 = torch.randn((K, T2, Mp), generator=gen, device=DEV)
    stack2[..., M:] = float('nan')
    tab2 = (torch.arange(B, device=DEV) * C).to(torch.int32)
    got2 = run_windows(stack2, T2, tab2, side[2])
    want2 = run_plain(stack2, side[3])
    assert torch.equal(got2[..., :Mo], want2[..., :Mo]), 'same memory, different result'
    assert torch.equal(side[2][..., :live], side[3][..., :live])
    # a table that breaks the caller's promise is held inside the stack: the windows at the two ends
    wild = starts.clone()
    wild[0], wild[B - 1] = T, -5
    clamped = run_windows(stack, T, wild, None)
    assert torch.equal(clamped[0, :, :Mo], got[0, :, :Mo])
    fixed = starts.clone()
    fixed[B - 1] = 0
    assert torch.equal(clamped[B - 1, :, :Mo], run_windows(stack, T, fixed, None)[B - 1, :, :Mo])
    # float64
    S = gathered[..., :M].permute(2, 0, 1, 3).reshape(C * K, B, M).double()          # rows c*K + k
    pre = torch.einsum('rbm,ro->bom', S, W.double())
    if bias_kind == VERTEX:
        pre = pre + bias[:, :M].double()
    elif bias_kind == FILTER:
        pre = pre + bias.double()[None, :, None]
    ref = _pool64(pre.clamp(min=0), pool, pool_kind)
    err = float((got[..., :Mo].double() - ref).abs().max() / pre.abs().max())
    record_measured('windows_kernel_vs_float64', B=B, M=M, C=C, K=K, Fout=Fout, pool=pool, pool_kind=pool_kind, bias_kind=bias_kind,
                    arm=arm, rel_err=err, bound=KREL)
    assert err <= KREL, '%s: %.3e' % (arm, err)


def test_every_served_arm_is_in_the_cases_and_unserved_shapes_say_so():
    lib = _lib.lib()
    assert {c[8] for c in KERNEL_CASES} == {RING, RINGP, SPLITK, PLAIN}
    for shape in ((64, 10466, 15, 5, 33, 1), (64, 10466, 15, 5, 64, 1), (64, 10466, 60, 5, 256, 1), (7, 360, 3, 3, 16, 16 * 3)):
        assert lib.chebgcn_contract_fwd_windows_supported(*shape) == 0, shape
    # not served: the status code, no launch
    buf = torch.zeros(1 << 16, device=DEV)
    tab = torch.zeros(4, dtype=torch.int32, device=DEV)
    rc = lib.chebgcn_contract_fwd_windows(P(buf), 8, P(tab), P(buf), None, 0, P(buf), None, 4, 32, 3, 2, 33, 1, 0, 1, stream())
    assert rc == -4


# ------------------------------------------------------------------------------------------------------------------------------
# end to end
# ------------------------------------------------------------------------------------------------------------------------------
SHARED = ('a3', 'a15', 'b', 'c_max', 'c_avg', 'c_maps')        # the shared path serves these; not 'wide' (64 filters), not the spectral filters
T_RUN = 40


def _series(name, seed=1, T=T_RUN):
    return np.random.RandomState(seed).randn(T, _laplacians(name)[0].shape[0]).astype(np.float32)


def _err(got, ref):
    d = np.abs(got.astype(np.float64) - ref).max(axis=1)
    return d / np.maximum(np.abs(ref).max(axis=1), 1e-30)


@pytest.mark.parametrize('name', sorted(NETS))
def test_decode_series_against_float64(name):
    net = _model(name)
    C = NETS[name]['channel']
    if name == 'b':
        assert net._relabelled
    if name == 'c_maps':
        assert net._pool_maps[0] is not None
    ref, Pm = _reference(name, net)
    series = _series(name)
    starts = decode.window_starts(T_RUN, C)
    want = reference_logits(ref, Pm, series, starts, C)
    bound = WIDE_REL if name == 'wide' else REL
    x = host_windows(series, starts, C)
    labels_predict = net.predict(x)
    top2 = np.sort(want, axis=1)[:, -2:]
    clear = (top2[:, 1] - top2[:, 0]) / np.abs(want).max(axis=1) > bound
    assert clear.sum() >= len(starts) // 2
    for share in ((True, False) if name in SHARED else (False,)):
        got = net.decode_series(series, share=share)
        assert net.last_decode_path == ('shared' if share else 'materialised')
        assert got.dtype == np.float32 and got.shape == want.shape
        e = _err(got, want)
        record_measured('decode_series_vs_float64', net=name, share=share, rel_err=float(e.max()), bound=bound, windows=len(starts))
        assert e.max() <= bound, '%s share=%s: %.3e' % (name, share, e.max())
        labels = net.decode_series(series, share=share, output='labels')
        assert labels.dtype == np.int64 and labels.shape == (len(starts),)
        assert np.array_equal(labels, got.argmax(axis=1))
        assert np.array_equal(labels[clear], want.argmax(axis=1)[clear])
        assert np.array_equal(labels[clear], labels_predict[clear].astype(np.int64))
        prob = net.decode_series(series, share=share, output='probabilities')
        z = got.astype(np.float64) - got.max(axis=1, keepdims=True)
        sm = np.exp(z) / np.exp(z).sum(axis=1, keepdims=True)
        assert prob.dtype == np.float32 and np.abs(prob - sm).max() <= 1e-6
    if name not in SHARED:
        with pytest.raises(ValueError, match='share=True'):
            net.decode_series(series, share=True)
        net.decode_series(series)                                 # 'auto' falls back by itself
        assert net.last_decode_path == 'materialised'


@pytest.mark.parametrize('name', ['a3', 'b', 'c_maps'])
def test_strides_starts_runs_and_short_runs(name):
    net = _model(name)
    C = NETS[name]['channel']
    ref, Pm = _reference(name, net)
    series = _series(name, seed=2)
    full = {share: net.decode_series(series, share=share) for share in (True, False)}
    for share in (True, False):
        for stride in (1, 2, C, C + 3):
            got = net.decode_series(series, stride=stride, share=share)
            st = np.arange(0, T_RUN - C + 1, stride)
            assert got.shape[0] == len(st)
            e = _err(got, reference_logits(ref, Pm, series, st, C))
            assert e.max() <= REL, (name, share, stride, e.max())
        st = np.array([T_RUN - C, 0, 7, 7, 3, T_RUN - C, 1])               # event-locked: unsorted, repeated, both ends
        got = net.decode_series(series, starts=st, share=share)
        assert _err(got, reference_logits(ref, Pm, series, st, C)).max() <= REL
        assert np.array_equal(got[2], got[3]) and np.array_equal(got[0], got[5])
        # a list of runs of different length, one of them exactly one window long; windows never cross runs
        runs = [series[:17], series[17:17 + C], series[20:]]
        outs = net.decode_series(runs, share=share, stride=2)
        assert isinstance(outs, list) and len(outs) == 3 and outs[1].shape[0] == 1
        for r, o in zip(runs, outs):
            st = np.arange(0, len(r) - C + 1, 2)
            assert o.shape[0] == len(st)
            assert _err(o, reference_logits(ref, Pm, r, st, C)).max() <= REL
        outs = net.decode_series(runs, starts=[[1, 0], [0], [2]], share=share)
        assert [o.shape[0] for o in outs] == [2, 1, 1]
        # any numeric dtype, or a tensor
        a = net.decode_series(series.astype(np.float64), share=share)
        b = net.decode_series(torch.as_tensor(series), share=share)
        assert np.array_equal(a, full[share]) and np.array_equal(b, full[share])
    with pytest.raises(ValueError, match='shorter'):
        net.decode_series(series[:C - 1])
    with pytest.raises(ValueError, match='start'):
        net.decode_series(series, starts=[T_RUN - C + 1])


@pytest.mark.parametrize('name', ['a3', 'b', 'c_avg'])
def test_chunked_batch_size_and_reruns_bit_identical(name):
    net = _model(name)
    C, K0 = NETS[name]['channel'], NETS[name]['K'][0]
    series = _series(name, seed=3, T=100)
    Mp = ops.plane_stride(series.shape[1])
    for share in (True, False):
        a = net.decode_series(series, share=share)
        assert np.array_equal(a, net.decode_series(series, share=share))
        for bs in (1, 7, 16):
            assert np.array_equal(a, net.decode_series(series, share=share, batch_size=bs)), (share, bs)
    whole = net.decode_series(series, share=True)
    timers = ops.KernelTimers()
    ops.timers = timers
    try:
        chunked = net.decode_series(series, share=True, max_stack_bytes=4 * K0 * Mp * 30)         # chunks of 30 time points
    finally:
        ops.timers = None
    plan = decode.chunk_plan(decode.window_starts(100, C), 100, C, 30)
    assert len(plan) >= 3
    sizes = {4.0 * series.shape[1] * (t1 - t0) * K0 for t0, t1, _ in plan}           # the recurrence's bytes over each chunk
    assert len([r for r in timers.records['recurrence_fwd'] if r[2] in sizes]) >= len(plan)
    assert not [r for r in timers.records['recurrence_fwd'] if r[2] == 4.0 * series.shape[1] * 100 * K0]
    assert np.array_equal(chunked, whole)
    st = np.array([90, 2, 50, 2, 31])
    assert np.array_equal(net.decode_series(series, starts=st, share=True, max_stack_bytes=4 * K0 * Mp * 30), whole[st])


@pytest.mark.parametrize('name', ['a3', 'b', 'c_max'])
def test_scale_and_shift_against_float64(name):
    net = _model(name)
    C = NETS[name]['channel']
    ref, Pm = _reference(name, net)
    series = _series(name, seed=4)
    rs = np.random.RandomState(5)
    M0 = series.shape[1]
    scale, shift = (0.5 + rs.rand(M0, C)).astype(np.float32), (0.3 * rs.randn(M0, C)).astype(np.float32)
    starts = decode.window_starts(T_RUN, C, stride=3)
    x = host_windows(series.astype(np.float64), starts, C)
    for sc, sh in ((scale, shift), (scale, None), (None, shift)):
        xs = x * (1.0 if sc is None else sc.astype(np.float64)) + (0.0 if sh is None else sh.astype(np.float64))
        ref.margin = None
        with torch.no_grad():
            want = ref.logits(Pm, torch.as_tensor(xs)).numpy()
        got = net.decode_series(series, stride=3, scale=sc, shift=sh)
        assert net.last_decode_path == 'materialised'
        e = _err(got, want)
        record_measured('decode_series_scaled_vs_float64', net=name, scale=sc is not None, shift=sh is not None, rel_err=float(e.max()))
        assert e.max() <= REL, (name, e.max())
        with pytest.raises(ValueError, match='share=True'):
            net.decode_series(series, scale=sc, shift=sh, share=True)


def test_shared_path_runs_one_recurrence_over_the_run_and_none_per_window():
    for name, fused in (('b', False), ('a3', True), ('c_maps', False)):
        net = _model(name)
        s = NETS[name]
        C, K0, M0 = s['channel'], s['K'][0], _laplacians(name)[0].shape[0]
        series = _series(name, seed=6)
        W = T_RUN - C + 1
        nb, nl = -(-W // BS), len(s['p'])
        timers = ops.KernelTimers()
        ops.timers = timers
        _lib.dispatch_log = log = []
        try:
            net.decode_series(series, share=True)
        finally:
            ops.timers, _lib.dispatch_log = None, None
        rec = timers.records
        assert len(rec['contract_fwd_windows']) == nb
        over_run = [r for r in rec['recurrence_fwd'] if r[2] == 4.0 * M0 * T_RUN * K0]
        assert len(over_run) == 1                                    # T planes, once
        # ... and no recurrence per batch of windows for the first layer: every other launch is one of the layers 2 .. n
        if fused:
            assert len(rec['recurrence_fwd']) == 1 and len(rec['fused_layer_fwd']) == nb * (nl - 1)
        else:
            assert len(rec['recurrence_fwd']) == 1 + nb * (nl - 1)
        assert {d for w, d in log if w == 'contract_fwd_windows'} == {'contract_fwd_windows_splitk_kernel'}
        if name == 'c_maps':
            assert len(rec['pool_gather_fwd']) == nb
        # the materialised path: a first-layer recurrence (or fused layer) per batch, no windowed contraction
        timers = ops.KernelTimers()
        ops.timers = timers
        try:
            net.decode_series(series, share=False)
        finally:
            ops.timers = None
        assert 'contract_fwd_windows' not in timers.records
        key = 'fused_layer_fwd' if fused else 'recurrence_fwd'
        assert len(timers.records[key]) == nb * nl


def test_auto_picks_by_model_windows_and_arguments():
    series = _series('b', seed=7)
    net = _model('b')                                                 # 1200 vertices: beyond the on-chip layer
    C = NETS['b']['channel']
    net.decode_series(series)
    assert net.last_decode_path == 'shared'
    net.decode_series(series, stride=C)                               # nothing overlaps: nothing to share
    assert net.last_decode_path == 'materialised'
    net.decode_series(series, starts=[0, C, 2 * C])
    assert net.last_decode_path == 'materialised'
    net.decode_series(series, starts=[0, 1])
    assert net.last_decode_path == 'shared'
    net.decode_series(series, scale=np.ones((series.shape[1], C), np.float32))
    assert net.last_decode_path == 'materialised'
    net.decode_series(series, share=False)
    assert net.last_decode_path == 'materialised'
    atlas = _model('a3')                                              # the atlas shape: 'auto' follows decode.AUTO_MIN_VERTICES
    atlas.decode_series(_series('a3'))
    assert atlas.last_decode_path == ('shared' if 360 >= decode.AUTO_MIN_VERTICES else 'materialised')
    k1 = models_gcn.cgcnn({'device': DEV}, _laplacians('b'), [6, 8], [1, 3], [1, 1], [9, 5], channel=2, batch_size=BS, verbose=False)
    with pytest.raises(ValueError, match='K\\[0\\]'):
        k1.decode_series(series, share=True)
    k1.decode_series(series)
    assert k1.last_decode_path == 'materialised'


def test_model_state_untouched_and_next_step_bit_identical():
    name = 'a3'
    x = np.random.RandomState(1).randn(BS, 360, 3).astype(np.float32)
    labels = torch.as_tensor(np.arange(BS) % 5, dtype=torch.int64, device=DEV)
    nets = [_model(name, seed=7), _model(name, seed=7)]
    for net in nets:
        net.enable_step_graph(True)
        xs = net._gather(net.stage(x), torch.arange(BS, dtype=torch.int32, device=DEV))
        for _ in range(3):
            net.train_step(xs, labels)          # two eager steps, then the captured one
        assert net._sg is not None
    a, b = nets
    torch.cuda.synchronize()
    assert _same(_state(a), _state(b))
    before, sg, grad_view = _state(a), a._sg, a.gradient('conv1/weights').clone()
    a.training_mode = True
    before[-1] = True
    series = _series(name, seed=8)
    a.decode_series(series, share=True)
    a.decode_series(series, share=False, batch_size=5, output='labels')
    a.decode_series([series, series[:9]], stride=2)
    torch.cuda.synchronize()
    assert _same(_state(a), before)
    assert a._sg is sg and a._step_graph_on and torch.equal(a.gradient('conv1/weights'), grad_view)
    assert a._windows is None and a._pass is None
    b.training_mode = True
    for net in nets:
        xs = net._gather(net.stage(x), torch.arange(BS, dtype=torch.int32, device=DEV))
        net.train_step(xs, labels)
    torch.cuda.synchronize()
    assert _same(_state(a), _state(b))


def test_model_perf_decode_series_from_fit_checkpoint(tmp_path, monkeypatch):
    name = 'a3'
    monkeypatch.setenv('CHEBGCN_HOME', str(tmp_path))
    xtr = np.random.RandomState(11).randn(16, 360, 3).astype(np.float32)
    ytr = np.arange(16) % 5
    net = _model(name, num_epochs=2, eval_frequency=2, dir_name='dec')
    net.fit(xtr, ytr, xtr[:8], ytr[:8])
    root = str(tmp_path) + '/checkpoints/dec'
    series = _series(name, seed=9)
    for kw in (dict(share=True), dict(share=False, output='labels'), dict(stride=2, output='probabilities')):
        got = models_gcn.model_perf().decode_series(root, series, batch_size=BS, **kw)
        live = models_gcn.model_perf._restore(root, BS, model=net)
        assert np.array_equal(got, live.decode_series(series, **kw))


def test_finetuning_cgcnn_decodes_on_both_paths(tmp_path, monkeypatch):
    name = 'c_max'
    s = NETS[name]
    monkeypatch.setenv('CHEBGCN_HOME', str(tmp_path))
    pre = _model(name, dir_name='pre')
    pre._save_best(50.0, 7, [])
    ft = models_gcn.finetuning_cgcnn({'device': DEV}, str(tmp_path) + '/checkpoints/', _laplacians(name), s['F'], s['K'],
                                     s['p'], [12, 5], channel=s['channel'], dir_name='pre', batch_size=BS, verbose=False,
                                     brelu=s['brelu'], pool=s['pool'])
    C = s['channel']
    series = _series(name, seed=10)
    starts = decode.window_starts(T_RUN, C)
    x = host_windows(series, starts, C)
    data = ft.stage(x)
    want = []
    ft.training_mode = False
    with torch.no_grad():
        for b0 in range(0, len(starts), BS):
            idx = torch.arange(b0, min(b0 + BS, len(starts)), dtype=torch.int32, device=DEV)
            want.append(ft._inference_storage(ft._gather(data, idx), 1).cpu().numpy())
    want = np.concatenate(want).astype(np.float64)
    for share in (True, False):
        got = ft.decode_series(series, share=share)
        assert ft.last_decode_path == ('shared' if share else 'materialised')
        e = _err(got, want)
        record_measured('decode_series_finetuning_vs_own_forward', share=share, rel_err=float(e.max()))
        assert e.max() <= REL, (share, e.max())
