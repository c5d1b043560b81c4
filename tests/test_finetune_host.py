"""Host side of ``finetuning_cgcnn`` (lib_new/models_gcn.py:685-933) on shape-only (meta) models: the checkpoint it reads,
the checks of its constructor, the variables it creates and their layout, its architecture record, the new ABI entries.
No GPU."""
import os

import numpy as np
import pytest
import torch

from conftest import ROOT
from gcn_fmri_decoding_amd import _lib, dist, graph, models_gcn

META = {'device': 'meta'}
F, K, P, CH = [4, 5, 6], [3, 3, 2], [1, 2, 2], 2


@pytest.fixture(scope='module')
def laplacians():
    Ls, _, _ = graph.synthetic_graph(100, k=6, levels=2, seed=1)
    return Ls


def _pretrained(tmp_path, Ls, F=F, K=K, p=P, channel=CH, name='pre', step=3, line1=None, **kw):
    """A checkpoint directory ``<tmp>/<name>/model/`` as cgcnn.fit writes it, holding a meta cgcnn's variables (zeros)."""
    net = models_gcn.cgcnn(META, Ls, F, K, p, [7, 3], channel=channel, verbose=False, **kw)
    sd = {'architecture': net._architecture(), 'global_step': step, 'names': net.variables()}
    for s in net._spec_list:
        sd[s.name] = torch.zeros(s.ref_shape)
    path = os.path.join(str(tmp_path), name, 'model')
    os.makedirs(path, exist_ok=True)
    torch.save(sd, os.path.join(path, 'best.ckpt-%d.pt' % step))
    with open(os.path.join(path, 'checkpoint'), 'w') as f:
        f.write('model_checkpoint_path: "%s"\n' % (line1 or 'best.ckpt-%d' % step))
        f.write('all_model_checkpoint_paths: "best.ckpt-%d"\n' % step)
    return str(tmp_path) + '/', sd


def _model(root, Ls, M=(9, 8, 4), **kw):
    args = dict(channel=CH, dir_name='pre', verbose=False)
    args.update(kw)
    return models_gcn.finetuning_cgcnn(META, root, Ls, kw.pop('F', F), kw.pop('K', K), kw.pop('p', P), list(M),
                                       **{k: v for k, v in args.items() if k not in ('F', 'K', 'p')})


def test_new_abi_entries_are_declared():
    header = open(os.path.join(ROOT, 'include', 'chebgcn.h')).read()
    for name in ('chebgcn_nadam_step_sq_all', 'chebgcn_planes_to_rows', 'chebgcn_rows_to_planes'):
        assert name in _lib.SIGNATURES
        assert name + '(' in header
    from gcn_fmri_decoding_amd.models_gcn import finetuning_cgcnn      # noqa: F401


def test_checkpoint_file_line_two_fallback(tmp_path, laplacians):
    root, _ = _pretrained(tmp_path, laplacians, step=3)
    path = root + 'pre/model/'
    assert models_gcn._saver_checkpoint(path) == path + 'best.ckpt-3.pt'
    _pretrained(tmp_path, laplacians, step=5)          # line 1 now names best.ckpt-5, which exists
    assert models_gcn._saver_checkpoint(path) == path + 'best.ckpt-5.pt'
    _pretrained(tmp_path, laplacians, step=3, line1='best.ckpt-9')      # line 1 names a file that is gone: line 2
    assert models_gcn._saver_checkpoint(path) == path + 'best.ckpt-3.pt'
    net = _model(root, laplacians)
    assert net.train_layers == []


def test_variables_names_shapes_and_layout(tmp_path, laplacians):
    root, sd = _pretrained(tmp_path, laplacians)
    net = _model(root, laplacians, initial=None)
    M_top = laplacians[1].shape[0]          # conv3 filters on level 1; the head reads it BEFORE its pooling (p = 2)
    want_head = [('newfc1/weights', (M_top * F[-1], 9)), ('newfc1/bias', (9,)), ('newfc2/weights', (9, 8)),
                 ('newfc2/bias', (8,)), ('newlogits/weights', (8, 4)), ('newlogits/bias', (4,))]
    specs = {s.name: s for s in net._spec_list}
    for name, shape in want_head:
        assert specs[name].ref_shape == shape
        assert specs[name].kind in ('normal', 'const')          # initial=None draws 'normal' (the reference raises)
    conv = [n for n in sd['names'] if n.startswith('conv')]      # the pretrained head (fc*, logits) is not taken
    assert sorted(net.variables()) == sorted(conv + [n for n, _ in want_head])
    for n in conv:
        assert specs[n].ref_shape == tuple(sd[n].shape)
    # only the variables this model creates are regularised; they are the head, first in the flat buffer
    assert net.regularizers == [n for n, _ in want_head]
    assert net.variables()[:6] == [n for n, _ in want_head]
    assert net._n_train == net._n_head == net._n_reg
    assert net._adam_m.numel() == net._n_train
    assert all(net._params[n].requires_grad == n.startswith('new') for n in net.variables())


@pytest.mark.parametrize('train_layers', [None, ['conv2'], ['conv1', 'conv3']])
def test_trainable_prefix(tmp_path, laplacians, train_layers):
    root, _ = _pretrained(tmp_path, laplacians)
    net = _model(root, laplacians, flag_tuning=True, train_layers=train_layers)
    want = [] if train_layers is None else train_layers       # the reference's conv4 ... conv6 do not exist here
    assert net.train_layers == want
    trained = [n for n in net.variables() if n.startswith('new') or n.split('/')[0] in want]
    assert net.variables()[:len(trained)] == trained or sorted(net.variables()[:len(trained)]) == sorted(trained)
    assert net._n_train == sum(int(np.prod(net._spec(n).shape)) for n in trained)
    assert all(net._slices[n][1] <= net._n_train for n in trained)
    assert all(net._params[n].requires_grad == (n in trained) for n in net.variables())
    assert net.regularizers == [n for n in net.variables() if n.startswith('new')]


def test_default_train_layers_on_six_layers(tmp_path):
    Ls, _, _ = graph.synthetic_graph(60, k=6, levels=0, seed=2)
    F6, K6, p6 = [3] * 6, [2] * 6, [1] * 6
    root, _ = _pretrained(tmp_path, Ls, F=F6, K=K6, p=p6, channel=1)
    net = models_gcn.finetuning_cgcnn(META, root, Ls, F6, K6, p6, [5, 3], dir_name='pre', flag_tuning=True, verbose=False)
    assert net.train_layers == ['conv4', 'conv5', 'conv6']
    assert net._lowest == 3
    frozen = models_gcn.finetuning_cgcnn(META, root, Ls, F6, K6, p6, [5, 3], dir_name='pre', verbose=False)
    assert frozen.train_layers == [] and frozen._lowest == 6


@pytest.mark.parametrize('what', ['F', 'K', 'p', 'channel', 'L'])
def test_mismatched_trunk_raises(tmp_path, laplacians, what):
    root, _ = _pretrained(tmp_path, laplacians)
    kw = {'F': [4, 5, 7], 'K': [3, 2, 2], 'p': [1, 1, 2], 'channel': 3}
    args = dict(F=F, K=K, p=P, channel=CH)
    Ls = laplacians
    if what == 'L':
        Ls = [laplacians[0][:90, :90]] + list(laplacians[1:])
    else:
        args[what] = kw[what]
    with pytest.raises(ValueError, match=what):
        models_gcn.finetuning_cgcnn(META, root, Ls, args['F'], args['K'], args['p'], [9, 4], channel=args['channel'],
                                    dir_name='pre', verbose=False)


def test_unsupported_trunk_and_arguments(tmp_path, laplacians):
    root, sd = _pretrained(tmp_path, laplacians)
    for key, value in (('filter', 'spline'), ('filter', 'chebyshev2'), ('pool', 'mpool2')):
        bad = dict(sd)
        bad['architecture'] = dict(sd['architecture'], **{key: value})
        torch.save(bad, root + 'pre/model/best.ckpt-3.pt')
        with pytest.raises(NotImplementedError, match=value):
            _model(root, laplacians)
    torch.save(sd, root + 'pre/model/best.ckpt-3.pt')
    with pytest.raises(ValueError, match='conv7'):
        _model(root, laplacians, flag_tuning=True, train_layers=['conv7'])
    with pytest.raises(ValueError, match='flag_tuning'):
        _model(root, laplacians, train_layers=['conv2'])
    net = _model(root, laplacians)
    with pytest.raises(NotImplementedError, match='finetuning_cgcnn'):
        dist.DataParallel(net)


def test_architecture_record_rebuilds_the_model(tmp_path, laplacians):
    root, _ = _pretrained(tmp_path, laplacians)
    net = _model(root, laplacians, flag_tuning=True, train_layers=['conv2', 'conv3'], regularization=5e-4, batch_size=16)
    arch = net._architecture()
    assert arch['class'] == 'finetuning_cgcnn' and arch['M'] == [9, 8, 4] and arch['train_layers'] == ['conv2', 'conv3']
    assert arch['trunk']['F'] == F and arch['trunk']['filter'] == 'chebyshev5' and len(arch['trunk']['L']) == len(laplacians)
    sd = {'architecture': arch, 'global_step': 4}
    for s in net._spec_list:
        sd[s.name] = torch.zeros(s.ref_shape)
    # the record alone rebuilds the model: the pretrained directory is gone
    os.remove(root + 'pre/model/best.ckpt-3.pt')
    again = models_gcn.finetuning_cgcnn.from_checkpoint(sd, config=META)
    assert again.variables() == net.variables()
    assert [again._spec(n).ref_shape for n in again.variables()] == [net._spec(n).ref_shape for n in net.variables()]
    assert again.train_layers == net.train_layers and again._n_train == net._n_train
    assert again.regularization == 5e-4 and again.batch_size == 16 and again.global_step == 4
