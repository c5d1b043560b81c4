"""MI355X-native Chebyshev graph convolution for fMRI decoding.

Drop-in for the hot path of zhangyu2ustc/GCN_fmri_decoding: ``lib_new.models_gcn.cgcnn``
(``chebyshev5`` / ``b1relu`` / ``b2relu`` / ``mpool1``), ``lib_new.graph`` (Laplacians)
and ``lib_new.coarsening`` (pooling index maps), on PyTorch-ROCm tensors, with the
arithmetic in hand-written gfx950 kernels behind the C ABI of ``include/chebgcn.h``.
"""
from . import _lib  # noqa: F401
from . import graph, coarsening, parcellation, filters, splits, stats, glm, searchlight, connectome, encoding  # noqa: F401
from .parcellation import Parcellation  # noqa: F401
from .filters import GraphFilter  # noqa: F401
from .stats import MapTestResult, map_test, map_test_host, sign_flips  # noqa: F401
from .stats import DesignTestResult, design_test, design_test_host, permutations, perm_t_host  # noqa: F401
from .glm import (Design, GLMResult, GLMResultAR1, contrasts_one_vs_rest, design_matrix, first_level,  # noqa: F401
                  first_level_host)
from .glm import TrialDesign, TrialResult, single_trial, single_trial_host, trial_design  # noqa: F401
# (the call itself is searchlight.searchlight: the package attribute stays the module)
from .searchlight import SearchlightResult, SolverInfo, lda_shrinkage_host, searchlight_events, searchlight_host  # noqa: F401
from .searchlight import RDMResult, compare_rdms, crossnobis, crossnobis_events, crossnobis_host  # noqa: F401
# (the call itself is connectome.connectome: the package attribute stays the module)
from .connectome import Connectome, connectome_host, Tangent, tangent, tangent_host  # noqa: F401
from .encoding import EncodingResult, delay_features, ridge_cv, ridge_cv_host  # noqa: F401

__all__ = ['graph', 'coarsening', 'parcellation', 'Parcellation', 'filters', 'GraphFilter', 'splits', 'stats', 'map_test',
           'map_test_host', 'sign_flips', 'MapTestResult', 'design_test', 'design_test_host', 'permutations', 'perm_t_host',
           'DesignTestResult', 'glm', 'Design', 'GLMResult', 'GLMResultAR1', 'design_matrix', 'contrasts_one_vs_rest',
           'first_level', 'first_level_host', 'TrialDesign', 'TrialResult', 'trial_design', 'single_trial', 'single_trial_host',
           'searchlight', 'SearchlightResult', 'SolverInfo', 'searchlight_events', 'searchlight_host',
           'lda_shrinkage_host', 'RDMResult', 'compare_rdms', 'crossnobis', 'crossnobis_events', 'crossnobis_host', 'connectome', 'Connectome',
           'connectome_host', 'Tangent', 'tangent', 'tangent_host', 'encoding', 'EncodingResult', 'delay_features', 'ridge_cv', 'ridge_cv_host',
           'models_gcn', 'ops']


def __getattr__(name):
    # torch-dependent modules are imported lazily so that the host-only parts
    # (graph, coarsening) stay importable in minimal environments
    if name in ('ops', 'models_gcn', 'dist'):
        import importlib
        return importlib.import_module('.' + name, __name__)
    raise AttributeError(name)
