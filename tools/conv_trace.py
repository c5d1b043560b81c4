#!/usr/bin/env python
"""What the graph-convolution layer launches, case by case: for a fixed list of seeded cases (single ``ops.cheb_conv`` layers,
``cgcnn`` / ``finetuning_cgcnn`` steps, forwards, window decodes and Grad-CAM passes) the ordered sequence of library entry
points called, the layer's ``(what, kernel templates)`` pairs of ``_lib.dispatch_log``, the number of ``ops._side_stream`` calls and
a SHA-256 over the bytes of every output and gradient (logical region only: plane padding excluded).

    python tools/conv_trace.py --out trace.json            # everything, hashes included
    python tools/conv_trace.py --golden                    # rewrites tests/golden/conv_dispatch.json (no hashes)

Two trees that launch the same kernels on the same operands in the same order write identical files on one machine: run it
on both sides of a change of ``ops.ChebConv`` / the models' trunk loop and compare.  The hashes are tied to a compiler and a
card, the sequences to the 256 CUs of an MI355X (the dispatchers choose by launch size); tests/test_gpu_conv_plan.py replays
the cases against the committed sequences.  It fails if an entry point of ``ENTRY_POINTS`` -- everything ``ChebConv`` and
``conv_windows`` can launch -- is reached by no case: a trace that misses an arm says nothing about it.

Shapes: batch 3, K = 3, at most 16 filters where the arm allows.  The arms that need more: the fused feature mean and the
gated contraction are not served to small launches (ceil(M / 512) * B < 2 * CUs), and the forward-form input gradient needs a
graph in length order, which the library serves from 1025 plane entries up -- those model cases run batch 176 on a 2550 / 1275
vertex pyramid; the bf16 dy16 kernels need Fin * K > 160 and Fout > 64 (40 -> 96 filters, K = 5)."""
import argparse
import contextlib
import hashlib
import json
import os
import shutil
import sys
import tempfile

import numpy as np
import scipy.sparse as sp
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from gcn_fmri_decoding_amd import _lib, graph, models_gcn, ops     # noqa: E402

GOLDEN = os.path.join(ROOT, 'tests', 'golden')
DEV = torch.device('cuda', 0)
SWITCHES = ('fold_relu_grad', 'dx_by_forward', 'bf16_dy16', 'fused_small', 'overlap_bwd_w', 'gate_links', 'merge_bias_small',
            'bias_side_small')
# every launching entry point of ChebConv.forward / backward and conv_windows (chebgcn_ + ...)
ENTRY_POINTS = (
    'recurrence_fwd', 'contract_fwd', 'contract_fwd_bf16', 'contract_fwd_gated', 'contract_fwd_mean', 'contract_fwd_windows',
    'pool_gather_fwd', 'fused_layer_fwd', 'relu_grad_mean', 'bias_grad_relu_mean', 'brelu_pool_bwd', 'relu_grad_bf16',
    'pool_scatter_bwd', 'contract_bwd_w', 'contract_bwd_w_relu', 'contract_bwd_w_relu_bias', 'contract_bwd_w_relu_mean',
    'contract_bwd_w_bf16', 'contract_bwd_w_bf16_dy16', 'fused_layer_bwd_x', 'recurrence_fwd_t', 'reindex_weights',
    'contract_bwd_x', 'contract_bwd_x_relu', 'contract_bwd_x_relu_mean', 'contract_bwd_x_bf16', 'contract_bwd_x_bf16_dy16',
    'recurrence_bwd')
ALSO_RECORDED = ('reindex_weights_batch',)           # the models' batched re-indexing: recorded, not part of the condition
# what ``ChebConv``, ``conv_windows`` and ``reindex_weights_batch`` hand to ``_lib.check``: the dispatch entries that are recorded.
# Every entry point behind them reports its own kernel templates.  The rest of a model's step is left out: some of its entry
# points (to_plane, feature_mean_fwd, ...) report none, and the log then repeats whatever the thread launched last -- the
# case before -- under their name.  Kept by hand beside ENTRY_POINTS: a new ``what`` string in ops.py that is not added here
# still shows in ``calls`` but is dropped from ``dispatch``.
LAYER_WHATS = frozenset((
    'recurrence_fwd', 'contract_fwd', 'contract_fwd_bf16', 'contract_fwd_mean', 'contract_fwd_windows', 'pool_gather_fwd',
    'fused_layer_fwd', 'relu_grad_mean', 'bias_grad_relu_mean', 'brelu_pool_bwd', 'relu_grad_bf16', 'pool_scatter_bwd',
    'contract_bwd_w', 'contract_bwd_w_bf16', 'contract_bwd_w_bf16x3', 'fused_layer_bwd_x', 'recurrence_fwd_t', 'reindex_weights',
    'contract_bwd_x', 'contract_bwd_x_bf16', 'contract_bwd_x_bf16x3', 'contract_bwd_x_relu', 'contract_bwd_x_relu_mean',
    'recurrence_bwd', 'reindex_weights_batch'))


def _csr(z, prefix):
    return sp.csr_matrix((z[prefix + '_data'], z[prefix + '_indices'], z[prefix + '_indptr']),
                         shape=tuple(int(s) for s in z[prefix + '_shape']))


class World:
    """Graphs and models the cases share, built on first use (outside the recording)."""

    def __init__(self):
        self._made, self._tmp = {}, None

    def get(self, name):
        if name not in self._made:
            self._made[name] = getattr(self, '_' + name)()
        return self._made[name]

    def close(self):
        self._made.clear()
        if self._tmp is not None:
            shutil.rmtree(self._tmp, ignore_errors=True)

    def _g100(self):                                 # atlas-sized: the fused on-chip layer serves it
        return ops.Graph(_csr(np.load(os.path.join(GOLDEN, 'graph_n100_f64.npz')), 'Ln').astype(np.float32), DEV)

    def _g900(self):                                 # too large for the fused layer, caller's vertex order
        rs = np.random.RandomState(4)
        N = 900
        A = sp.random(N, N, density=6.0 / N, random_state=rs, format='csr', dtype=np.float32)
        A = A + A.T
        A.setdiag(0)
        A.eliminate_zeros()
        return ops.Graph(graph.laplacian(A.tocsr(), normalized=True), DEV)

    def _pyr512(self):                               # 592 / 296 / 148 vertices
        z = np.load(os.path.join(GOLDEN, 'coarsen_n512.npz'))
        return [graph.laplacian(_csr(z, 'graph%d' % i).astype(np.float32), normalized=True) for i in range(3)]

    def _pyr2400(self):                              # 2550 / 1275 vertices: both levels get the length order
        return graph.synthetic_graph(2400, k=6, levels=1, seed=3)[0]

    def _g1275(self):                                # one level of it in length order, for a lone forward-form layer
        L = self.get('pyr2400')[1]
        g = ops.Graph(L, DEV, order=graph.length_order(L))
        assert g.ordered, 'the ordered recurrence does not serve the 1275-vertex level'
        return g

    def _cgcnn(self, Ls, batch, seed=0, **kw):
        torch.manual_seed(seed)
        net = models_gcn.cgcnn({'device': DEV}, Ls, [8, 8, 8], [3, 3, 3], [2, 1, 1], [12, 5], channel=4, brelu='b2relu',
                               batch_size=batch, regularization=5e-4, dropout=1, verbose=False, **kw)
        net.contraction = 'f32'
        return net

    def _net512(self):
        return self._cgcnn(self.get('pyr512'), 3)

    def _net2400(self):
        return self._cgcnn(self.get('pyr2400'), 176)

    def _ckpt(self):                                 # a cgcnn checkpoint as fit() saves it, for the fine-tuning models
        self._tmp = tempfile.mkdtemp(prefix='conv_trace_')
        home = os.environ.get('CHEBGCN_HOME')
        os.environ['CHEBGCN_HOME'] = self._tmp
        try:
            self._cgcnn(self.get('pyr512'), 3, seed=5, dir_name='pre')._save_best(50.0, 7, [])
        finally:
            if home is None:
                del os.environ['CHEBGCN_HOME']
            else:
                os.environ['CHEBGCN_HOME'] = home
        return self._tmp + '/checkpoints/'

    def _ft(self, **kw):
        torch.manual_seed(1)
        net = models_gcn.finetuning_cgcnn({'device': DEV}, self.get('ckpt'), self.get('pyr512'), [8, 8, 8], [3, 3, 3], [2, 1, 1],
                                          [12, 5], channel=4, brelu='b2relu', dir_name='pre', verbose=False, regularization=1e-3,
                                          batch_size=3, **kw)
        net.contraction = 'f32'
        return net

    def _ft_top2(self):
        return self._ft(flag_tuning=True, train_layers=['conv2', 'conv3'])

    def _ft_frozen(self):
        return self._ft()


# ------------------------------------------------------------------------------------ the cases

def _layer(world, gname, Fin, Fout, K=3, B=3, seed=0, x_grad=True, w_grad=True, maps=False, **kw):
    """One cheb_conv layer, forward and backward: outputs and gradients by name."""
    g = world.get(gname)
    M = g.M
    rs = np.random.RandomState(seed)
    pool = kw.get('pool', 1)
    x = torch.zeros((B, Fin, g.Mp), device=DEV)
    x[..., :M] = torch.as_tensor(rs.randn(B, Fin, M).astype(np.float32)).to(DEV)
    W = torch.as_tensor((rs.randn(Fin * K, Fout) * 0.1).astype(np.float32)).to(DEV)
    kind = kw.get('bias_kind', ops.BIAS_NONE)
    b = None
    if kind == ops.BIAS_VERTEX:
        b = torch.zeros((Fout, g.Mp), device=DEV)
        b[:, :M] = torch.as_tensor((rs.randn(Fout, M) * 0.1).astype(np.float32)).to(DEV)
    elif kind == ops.BIAS_FILTER:
        b = torch.as_tensor((rs.randn(Fout) * 0.1).astype(np.float32)).to(DEV)
    if maps:
        kw['pool_maps'] = ops.pool_maps(pool, rs.permutation(M), rs.permutation(M // pool), M, DEV)
    x.requires_grad_(x_grad)
    W.requires_grad_(w_grad)
    if b is not None:
        b.requires_grad_(True)
    Mo = M // pool
    out = ops.cheb_conv(x, W, b, g, K, **kw)
    gout = torch.zeros_like(out)
    gout[..., :Mo] = torch.as_tensor(rs.randn(B, Fout, Mo).astype(np.float32)).to(DEV)
    out.backward(gout)
    res = {'out': out.detach()[..., :Mo]}
    if x_grad:
        res['dx'] = x.grad[..., :M]
    if w_grad:
        res['dW'] = W.grad
    if b is not None:
        res['dbias'] = b.grad[:, :M] if kind == ops.BIAS_VERTEX else b.grad
    return res


def _batch(net, B, seed=2):
    rs = np.random.RandomState(seed)
    x = rs.randn(B, net.L[0].shape[0], int(net.channel)).astype(np.float32)
    labels = torch.as_tensor(rs.randint(0, int(net.M[-1]), B), dtype=torch.int64, device=DEV)
    return x, ops.plane_storage(torch.as_tensor(x).to(DEV)), labels


def _step(world, name, B):
    """One training step of a model made afresh from its own start values: every variable after it and every gradient."""
    net = world.get(name)
    if not hasattr(net, '_trace_start'):
        net._trace_start = net._flat.detach().clone()
    with torch.no_grad():
        net._flat.copy_(net._trace_start)
        net._grad.zero_()
    _, xs, labels = _batch(net, B)
    _, loss = net.train_step(xs, labels)
    res = {'loss': loss.detach().reshape(1)}
    for k in net.variables():
        res['var:' + k] = torch.as_tensor(net.get_var(k))
        if net._params[k].requires_grad:
            res['grad:' + k] = net.gradient(k)
    return res


def _forward(world, name, B):
    net = world.get(name)
    x, _, _ = _batch(net, B)
    with torch.no_grad():
        return {'logits': net.inference(torch.as_tensor(x).to(DEV), 1)}


def _decode(world, name):
    net = world.get(name)
    series = np.random.RandomState(6).randn(12, net.L[0].shape[0]).astype(np.float32)
    return {'logits': torch.as_tensor(net.decode_series(series, share=True, batch_size=3))}


def _gradcam(world, name):
    net = world.get(name)
    x, _, _ = _batch(net, 3)
    cam, target = net.gradcam(x, layer='conv2', batch_size=3)
    return {'cam': torch.as_tensor(cam), 'target': torch.as_tensor(np.asarray(target))}


V, F_ = ops.BIAS_VERTEX, ops.BIAS_FILTER
WIDE = dict(Fin=40, Fout=96, K=5, relu=True, bias_kind=V)
CASES = [
    # (name, the graph or model it runs on, switches, run)
    ('fused_vertex_bias', 'g100', {}, lambda w: _layer(w, 'g100', 8, 8, relu=True, bias_kind=V)),
    ('fused_vertex_bias_no_merge', 'g100', {'merge_bias_small': False}, lambda w: _layer(w, 'g100', 8, 8, relu=True, bias_kind=V)),
    ('fused_filter_bias', 'g100', {}, lambda w: _layer(w, 'g100', 8, 16, relu=True, bias_kind=F_)),
    ('fused_filter_bias_side', 'g100', {'overlap_bwd_w': True}, lambda w: _layer(w, 'g100', 8, 16, relu=True, bias_kind=F_)),
    ('fused_frozen_weight', 'g100', {}, lambda w: _layer(w, 'g100', 8, 8, relu=True, bias_kind=V, w_grad=False)),
    ('fused_no_relu', 'g100', {}, lambda w: _layer(w, 'g100', 8, 8, relu=False, bias_kind=F_)),
    ('unfused_atlas', 'g100', {'fused_small': False}, lambda w: _layer(w, 'g100', 8, 8, relu=True, bias_kind=V)),
    ('fold_clenshaw', 'g900', {}, lambda w: _layer(w, 'g900', 8, 16, relu=True, bias_kind=V)),
    ('fold_off', 'g900', {'fold_relu_grad': False}, lambda w: _layer(w, 'g900', 8, 16, relu=True, bias_kind=V)),
    ('no_input_grad', 'g900', {}, lambda w: _layer(w, 'g900', 8, 16, relu=True, bias_kind=F_, x_grad=False)),
    ('frozen_weight', 'g900', {}, lambda w: _layer(w, 'g900', 8, 16, relu=True, bias_kind=F_, w_grad=False)),
    ('pool2_max_relu', 'g900', {}, lambda w: _layer(w, 'g900', 8, 16, pool=2, pool_kind=ops.POOL_MAX, relu=True, bias_kind=V)),
    ('pool2_max', 'g900', {}, lambda w: _layer(w, 'g900', 8, 16, pool=2, pool_kind=ops.POOL_MAX, relu=False, bias_kind=F_)),
    ('pool2_avg_relu', 'g900', {}, lambda w: _layer(w, 'g900', 8, 16, pool=2, pool_kind=ops.POOL_AVG, relu=True, bias_kind=F_)),
    ('pool2_avg', 'g900', {}, lambda w: _layer(w, 'g900', 8, 16, pool=2, pool_kind=ops.POOL_AVG, relu=False)),
    ('pool2_maps', 'g900', {}, lambda w: _layer(w, 'g900', 8, 16, pool=2, pool_kind=ops.POOL_MAX, relu=True, bias_kind=V, maps=True)),
    ('bf16_dy16', 'g900', {}, lambda w: _layer(w, 'g900', precision='bf16', **WIDE)),
    ('bf16_dy32', 'g900', {'bf16_dy16': False}, lambda w: _layer(w, 'g900', precision='bf16', **WIDE)),
    ('bf16x3', 'g900', {}, lambda w: _layer(w, 'g900', precision='bf16x3', **WIDE)),
    ('bf16x3_side_off', 'g900', {'overlap_bwd_w': False}, lambda w: _layer(w, 'g900', precision='bf16x3', **WIDE)),
    ('forward_form_layer', 'g1275', {}, lambda w: _layer(w, 'g1275', 16, 8, relu=True, bias_kind=V)),
    ('cgcnn_step', 'net2400', {}, lambda w: _step(w, 'net2400', 176)),
    ('cgcnn_step_clenshaw', 'net2400', {'dx_by_forward': False}, lambda w: _step(w, 'net2400', 176)),
    ('cgcnn_step_no_links', 'net2400', {'gate_links': False}, lambda w: _step(w, 'net2400', 176)),
    ('cgcnn_step_no_fold', 'net2400', {'fold_relu_grad': False}, lambda w: _step(w, 'net2400', 176)),
    ('cgcnn_step_side', 'net2400', {'overlap_bwd_w': True}, lambda w: _step(w, 'net2400', 176)),
    ('cgcnn_step_pyramid512', 'net512', {}, lambda w: _step(w, 'net512', 3)),
    ('finetune_step_top2', 'ft_top2', {}, lambda w: _step(w, 'ft_top2', 3)),
    ('finetune_step_frozen', 'ft_frozen', {}, lambda w: _step(w, 'ft_frozen', 3)),
    ('cgcnn_no_grad', 'net512', {}, lambda w: _forward(w, 'net512', 3)),
    ('finetune_no_grad', 'ft_top2', {}, lambda w: _forward(w, 'ft_top2', 3)),
    ('cgcnn_windows', 'net512', {}, lambda w: _decode(w, 'net512')),
    ('cgcnn_windows_relabelled', 'net2400', {}, lambda w: _decode(w, 'net2400')),      # pools through index maps
    ('finetune_windows', 'ft_top2', {}, lambda w: _decode(w, 'ft_top2')),
    ('cgcnn_gradcam', 'net512', {}, lambda w: _gradcam(w, 'net512')),
    ('finetune_gradcam', 'ft_top2', {}, lambda w: _gradcam(w, 'ft_top2')),
]


# ------------------------------------------------------------------------------------ recording

@contextlib.contextmanager
def recording(switches):
    """The ``ops`` switches set for one case; inside: every call of a listed entry point, the dispatch log, the side streams."""
    lib = _lib.lib()
    rec = {'calls': [], 'side_streams': 0}
    saved = {k: getattr(ops, k) for k in SWITCHES}
    entries = {'chebgcn_' + n: getattr(lib, 'chebgcn_' + n) for n in ENTRY_POINTS + ALSO_RECORDED}
    side = ops._side_stream

    def counted(name, fn):
        def call(*args):
            rec['calls'].append(name[len('chebgcn_'):])
            return fn(*args)
        return call

    def side_stream(dev):
        rec['side_streams'] += 1
        return side(dev)

    try:
        for k, v in switches.items():
            setattr(ops, k, v)
        for name, fn in entries.items():
            setattr(lib, name, counted(name, fn))
        ops._side_stream = side_stream
        _lib.dispatch_log = []
        yield rec
        torch.cuda.synchronize()
        rec['dispatch'] = [[what, name] for what, name in _lib.dispatch_log if what in LAYER_WHATS]
    finally:
        _lib.dispatch_log = None
        ops._side_stream = side
        for name, fn in entries.items():
            setattr(lib, name, fn)
        for k, v in saved.items():
            setattr(ops, k, v)


def run_case(world, name, hashes=True):
    """{'calls', 'dispatch', 'side_streams'[, 'sha256']} of one case."""
    part, switches, fn = next((p, s, f) for n, p, s, f in CASES if n == name)
    world.get(part)                                  # built outside the recording
    with recording(switches) as rec:
        res = fn(world)
    if hashes:
        h = hashlib.sha256()
        for key in sorted(res):
            t = res[key].detach().contiguous().cpu()
            h.update(key.encode())
            h.update(str(tuple(t.shape)).encode())
            h.update(t.view(torch.uint8).numpy().tobytes() if t.numel() else b'')
        rec['sha256'] = h.hexdigest()
    return rec


def missing_entry_points(records):
    seen = set()
    for rec in records.values():
        seen.update(rec['calls'])
    return [n for n in ENTRY_POINTS if n not in seen]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--out', default=None, help='write the full trace (hashes included) here')
    ap.add_argument('--golden', action='store_true', help='rewrite tests/golden/conv_dispatch.json (sequences and counts only)')
    args = ap.parse_args()
    world = World()
    try:
        records = {name: run_case(world, name) for name, _, _, _ in CASES}
    finally:
        world.close()
    for name, rec in records.items():
        print('%-28s %3d calls, %d side streams  %s' % (name, len(rec['calls']), rec['side_streams'], ' '.join(sorted(set(rec['calls'])))))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(records, f, indent=1, sort_keys=True)
    if args.golden:
        with open(os.path.join(GOLDEN, 'conv_dispatch.json'), 'w') as f:
            json.dump({n: {k: v for k, v in r.items() if k != 'sha256'} for n, r in records.items()}, f, indent=1, sort_keys=True)
    missing = missing_entry_points(records)
    if missing:
        print('entry points no case reaches: %s' % ', '.join(missing))
        return 1
    return 0


if __name__ == '__main__':
    sys.exit(main())
