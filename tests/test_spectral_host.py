"""Host side of the spectral filters (cgcnn filter='fourier' / 'spline', lib_new/models_gcn.py:512-556) against the
reference's own outputs (tests/golden/inference_{fourier,spline}_n*.npz, written by tools/gen_spectral_golden.py): the
Fourier basis, the B-spline basis, and the variables the two models create.  No GPU."""
import numpy as np
import pytest

from conftest import csr_from, load_golden
from gcn_fmri_decoding_amd import graph as graph_mod
from gcn_fmri_decoding_amd import models_gcn

CASES = ['inference_fourier_n100', 'inference_fourier_n100_p21', 'inference_spline_n100', 'inference_spline_n100_p21']


def _layer_levels(p):
    """Graph level of each conv layer (the level advances by log2(p), models_gcn.py:462-469)."""
    out, j = [], 0
    for pp in p:
        out.append(j)
        j += int(np.log2(pp)) if pp > 1 else 0
    return out


@pytest.mark.parametrize('name', CASES)
def test_fourier_basis_matches_reference(name):
    z = load_golden(name)
    same_numpy = str(z['numpy_version']) == np.__version__
    for i in range(int(z['nlevels'])):
        lamb, U = graph_mod.fourier(csr_from(z, 'L%d' % i))
        assert lamb.dtype == np.float32 and U.dtype == np.float32      # a float32 Laplacian: a float32 decomposition
        assert np.all(np.diff(lamb) > 0)
        assert np.abs(lamb - z['lamb%d' % i]).max() <= 1e-6
        Uref = z['U%d' % i]
        sign = np.where(np.sum(U * Uref, axis=0) < 0, -1.0, 1.0).astype(np.float32)
        if same_numpy:
            assert np.array_equal(U * sign, Uref)
        else:
            assert np.abs(U * sign - Uref).max() <= 1e-3


@pytest.mark.parametrize('name', ['inference_spline_n100', 'inference_spline_n100_p21'])
def test_bspline_basis_bit_exact(name):
    z = load_golden(name)
    levels = _layer_levels(z['p'].tolist())
    for i, K in enumerate(z['K'].tolist()):
        B = models_gcn.bspline_basis(K, z['lamb%d' % levels[i]], degree=3)
        ref = z['B%d' % i]
        assert B.shape == ref.shape == (z['lamb%d' % levels[i]].shape[0], K)
        assert B.dtype == ref.dtype
        assert np.array_equal(B, ref)


def test_bspline_basis_evenly_spaced_points():
    B = models_gcn.bspline_basis(6, 50)
    assert B.shape == (50, 6)
    assert np.allclose(B.sum(axis=1), 1.0)          # partition of unity (the last point via basis[-1, -1] = 1)
    assert B[-1, -1] == 1


def _meta_model(z, **kw):
    Ls = [csr_from(z, 'L%d' % i) for i in range(int(z['nlevels']))]
    return models_gcn.cgcnn({'device': 'meta'}, Ls, z['F'].tolist(), z['K'].tolist(), z['p'].tolist(), z['M'].tolist(),
                            filter=str(z['filter']), brelu=str(z['brelu']), channel=int(z['channel']),
                            batch_size=int(z['x'].shape[0]), verbose=False, **kw)


@pytest.mark.parametrize('name', CASES)
def test_variable_names_and_shapes(name):
    z = load_golden(name)
    net = _meta_model(z)
    ref = {k[len('param:'):]: tuple(z[k].shape) for k in z.files if k.startswith('param:')}
    got = {n: net._spec(n).ref_shape for n in net.variables()}
    assert got == ref
    spline = str(z['filter']) == 'spline'
    F, K, Fin = z['F'].tolist(), z['K'].tolist(), [int(z['channel'])] + z['F'].tolist()[:-1]
    for i in range(len(F)):
        w = 'conv%d/weights' % (i + 1)
        M = net.L[i].shape[0]
        assert got[w] == ((K[i], F[i] * Fin[i]) if spline else (M, F[i], Fin[i]))
        # spline weights are not regularised (models_gcn.py:552), Fourier weights are (:536)
        assert (w in net.regularizers) == (not spline)


def test_spline_weights_sit_behind_the_regularised_prefix():
    z = load_golden('inference_spline_n100')
    net = _meta_model(z, regularization=5e-4)
    names = [s.name for s in net._spec_list]
    reg = [s.regularized for s in net._spec_list]
    assert reg == sorted(reg, reverse=True)          # every regularised variable before every other one
    assert not any(n.startswith('conv') for n, r in zip(names, reg) if r)
    assert net._n_reg == sum(int(np.prod(s.shape)) for s in net._spec_list if s.regularized)


def test_he_fan_in_of_fourier_weights():
    z = load_golden('inference_fourier_n100')
    net = _meta_model(z, initial='he')
    s = net._spec('conv1/weights')
    assert s.fan_in == s.shape[0] * s.shape[1]        # TF: prod(shape[:-1]) for a rank-3 variable
    assert net._spec('fc1/weights').fan_in == net._spec('fc1/weights').shape[0]


def test_basis_is_computed_through_graph_fourier(monkeypatch):
    z = load_golden('inference_fourier_n100_p21')
    calls = []
    real = graph_mod.fourier

    def spy(L, *a, **kw):
        calls.append(L.shape[0])
        return real(L, *a, **kw)
    monkeypatch.setattr(graph_mod, 'fourier', spy)
    _meta_model(z)
    assert sorted(calls) == [50, 100]                 # once per distinct Laplacian
