"""ctypes binding of libchebgcn.so (include/chebgcn.h).

The library is the product: there is no CPU or PyTorch fallback.  If the shared object
is missing or a call fails, an exception is raised -- never a silent alternative path.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('CHEBGCN_LIB') or os.path.join(_HERE, 'libchebgcn.so')   # override: kernel experiments only

BIAS_NONE, BIAS_FILTER, BIAS_VERTEX = 0, 1, 2
POOL_MAX, POOL_AVG = 0, 1
KNN_EUCLIDEAN, KNN_COSINE, KNN_CORRELATION, KNN_DOT = 0, 1, 2, 3
KNN_KMAX = 32
MC_SITES = 16
PARCEL_MEAN, PARCEL_SUM = 0, 1
FILTER_AUTO, FILTER_ROLLING, FILTER_STACK = 0, 1, 2
FILTER_JMAX, FILTER_KMAX = 8, 256
CLUSTER_MAX, CLUSTER_EXTENT, CLUSTER_TFCE = 0, 1, 2
CLUSTER_AUTO, CLUSTER_ONCHIP, CLUSTER_STREAMED = 0, 1, 2
CLUSTER_EHEIGHTS, CLUSTER_ELOOP = 1, 2
CONNECTOME_KINDS = ('covariance', 'correlation', 'precision', 'partial correlation')      # CHEBGCN_CONNECTOME_* in this order
SYM_FUNCTIONS = ('log', 'exp', 'sqrt', 'rsqrt')                                             # CHEBGCN_SYM_* in this order
RIDGE_SCORES = ('r2', 'r')                                                                  # CHEBGCN_RIDGE_* in this order


class ChebgcnError(RuntimeError):
    pass


_p = C.c_void_p
_i = C.c_int
_i64 = C.c_int64
_f = C.c_float

# name -> (restype, argtypes); mirrors include/chebgcn.h one to one
SIGNATURES = {
    'chebgcn_version': (_i, []),
    'chebgcn_last_error': (C.c_char_p, []),
    'chebgcn_last_dispatch': (C.c_char_p, []),
    'chebgcn_plane_stride': (_i, [_i]),
    'chebgcn_graph_create': (_i, [_i, _i64, _p, _p, _p, C.POINTER(_p)]),
    'chebgcn_graph_create_planes': (_i, [_i, _i64, _p, _p, _p, _i, C.POINTER(_p)]),
    'chebgcn_graph_destroy': (None, [_p]),
    'chebgcn_graph_query': (_i, [_p, _i, C.POINTER(_i64)]),
    'chebgcn_recurrence_fwd': (_i, [_p, _p, _p, _i, _i, _i, _p]),
    'chebgcn_recurrence_bwd': (_i, [_p, _p, _p, _i, _i, _i, _p]),
    'chebgcn_recurrence_fwd_t': (_i, [_p, _p, _p, _i, _i, _i, _p]),
    'chebgcn_reindex_weights': (_i, [_p, _p, _i, _i, _i, _p]),
    'chebgcn_reindex_weights_batch': (_i, [_i, _p, _p, _p, _p, _p, _p]),
    'chebgcn_contract_fwd': (_i, [_p, _p, _p, _i, _p, _p, _i, _i, _i, _i, _i, _i, _i, _i, _p]),
    'chebgcn_contract_fwd_windows_supported': (_i, [_i, _i, _i, _i, _i, _i]),
    'chebgcn_contract_fwd_windows': (_i, [_p, _i64, _p, _p, _p, _i, _p, _p, _i, _i, _i, _i, _i, _i, _i, _i, _p]),
    'chebgcn_contract_fwd_bf16_workspace': (C.c_size_t, [_i, _i, _i]),
    'chebgcn_contract_fwd_bf16': (_i, [_p, _p, _p, _i, _p, _p, _i, _i, _i, _i, _i, _i, _i, _i, _i, _p, C.c_size_t, _p]),
    'chebgcn_contract_bwd_x_bf16_workspace': (C.c_size_t, [_i, _i, _i]),
    'chebgcn_contract_bwd_x_bf16': (_i, [_p, _p, _p, _i, _i, _i, _i, _i, _i, _p, C.c_size_t, _p]),
    'chebgcn_contract_bwd_w_bf16_workspace': (C.c_size_t, [_i, _i, _i, _i, _i]),
    'chebgcn_contract_bwd_w_bf16': (_i, [_p, _p, _p, _p, C.c_size_t, _i, _i, _i, _i, _i, _i, _p]),
    'chebgcn_adam_partials': (_i, [_i64]),
    'chebgcn_adam_step_sq': (_i, [_p, _p, _p, _p, _i64, _f, _p, _f, _f, _f, _f, _f, _p, _p]),
    'chebgcn_adam_step_sq_all': (_i, [_p, _p, _p, _p, _i64, _i64, _f, _p, _f, _f, _f, _f, _f, _p, _p]),
    'chebgcn_nadam_step_sq_all': (_i, [_p, _p, _p, _p, _i64, _i64, _f, _p, _f, _f, _f, _f, _f, _p, _p]),
    'chebgcn_loss_bookkeeping': (_i, [_p, _p, _i, _f, _p, _f, _f, _p, _p, _p, _p]),
    'chebgcn_set_scalars': (_i, [_p, C.c_float, C.c_float, _p]),
    'chebgcn_softmax_xent': (_i, [_p, _p, _i, _p, _p, _i, _i, _p]),
    'chebgcn_relu_grad_bf16': (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _p, C.c_size_t, _p]),
    'chebgcn_bf16_dy16_supported': (_i, [_i, _i, _i, _i, _i]),
    'chebgcn_contract_bwd_w_bf16_dy16': (_i, [_p, _p, _p, _p, C.c_size_t, _i, _i, _i, _i, _i, _p]),
    'chebgcn_contract_bwd_x_bf16_dy16': (_i, [_p, _p, _p, _i, _i, _i, _i, _i, _p, C.c_size_t, _p]),
    'chebgcn_brelu_pool_fwd': (_i, [_p, _p, _i, _p, _p, _i, _i, _i, _i, _i, _i, _p]),
    'chebgcn_brelu_pool_bwd_workspace': (C.c_size_t, [_i, _i, _i, _i, _i]),
    'chebgcn_brelu_pool_bwd': (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _p, C.c_size_t, _p]),
    'chebgcn_pool_gather_fwd': (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _p]),
    'chebgcn_pool_scatter_bwd_workspace': (C.c_size_t, [_i, _i, _i, _i, _i]),
    'chebgcn_pool_scatter_bwd': (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _p, C.c_size_t, _p]),
    'chebgcn_contract_bwd_w_workspace': (C.c_size_t, [_i, _i, _i, _i, _i]),
    'chebgcn_contract_bwd_w': (_i, [_p, _p, _p, _p, C.c_size_t, _i, _i, _i, _i, _i, _p]),
    'chebgcn_contract_bwd_x': (_i, [_p, _p, _p, _i, _i, _i, _i, _i, _p]),
    'chebgcn_contract_bwd_x_relu': (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _i, _p]),
    'chebgcn_contract_bwd_w_relu': (_i, [_p, _p, _p, _p, _p, C.c_size_t, _i, _i, _i, _i, _i, _p]),
    'chebgcn_contract_bwd_w_relu_bias_merged': (_i, [_i, _i, _i, _i, _i]),
    'chebgcn_contract_bwd_w_relu_bias': (_i, [_p, _p, _p, _p, _p, _p, C.c_size_t, _i, _i, _i, _i, _i, _p]),
    'chebgcn_contract_fwd_mean_supported': (_i, [_i, _i, _i, _i, _i]),
    'chebgcn_contract_fwd_gated_supported': (_i, [_i, _i, _i, _i, _i]),
    'chebgcn_contract_fwd_gated': (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _i, _p]),
    'chebgcn_contract_fwd_mean': (_i, [_p, _p, _p, _i, _p, _p, _i, _i, _i, _i, _i, _p]),
    'chebgcn_contract_bwd_w_relu_mean': (_i, [_p, _p, _p, _p, _p, C.c_size_t, _i, _i, _i, _i, _i, _p]),
    'chebgcn_contract_bwd_x_relu_mean': (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _i, _p]),
    'chebgcn_bias_grad_relu_mean': (_i, [_p, _p, _p, _i, _i, _i, _i, _p, C.c_size_t, _p]),
    'chebgcn_relu_grad_mean': (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _p, C.c_size_t, _p]),
    'chebgcn_fused_layer_supported': (_i, [_p, _i, _i, _i, _i]),
    'chebgcn_fused_layer_workspace': (C.c_size_t, [_p, _i, _i, _i, _i]),
    'chebgcn_fused_layer_fwd': (_i, [_p, _p, _p, _p, _i, _p, _p, _p, _p, C.c_size_t, _i, _i, _i, _i, _i, _p]),
    'chebgcn_fused_layer_bwd_x': (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _i, _p]),
    'chebgcn_perm_data': (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _p]),
    'chebgcn_to_plane': (_i, [_p, _p, _i, _i, _i, _p]),
    'chebgcn_from_plane': (_i, [_p, _p, _i, _i, _i, _p]),
    'chebgcn_feature_mean_fwd': (_i, [_p, _p, _i, _i, _i, _p]),
    'chebgcn_feature_mean_bwd': (_i, [_p, _p, _i, _i, _i, _p]),
    'chebgcn_fc_fwd_supported': (_i, [_i, _i, _i]),
    'chebgcn_fc_fwd_workspace': (C.c_size_t, [_i, _i, _i]),
    'chebgcn_fc_fwd': (_i, [_p, _i64, _p, _p, _p, _p, C.c_size_t, _i, _i, _i, _i, _p]),
    'chebgcn_fc_bwd': (_i, [_p, _i64, _p, _p, _p, _p, _p, _p, _i64, _i, _i, _i, _p]),
    'chebgcn_planes_to_rows': (_i, [_p, _p, _p, _i, _i, _i, _i64, _p]),
    'chebgcn_rows_to_planes': (_i, [_p, _p, _p, _i, _i, _i, _i64, _p]),
    'chebgcn_adam_step': (_i, [_p, _p, _p, _p, _i64, _f, _f, _f, _f, _f, _f, _p]),
    'chebgcn_adam_step_dev': (_i, [_p, _p, _p, _p, _i64, _p, _f, _f, _f, _f, _f, _p]),
    'chebgcn_metis_one_level_f32': (_i, [_i64, _p, _p, _p, _p, _p, _i64, _p]),
    'chebgcn_metis_one_level_f32p': (_i, [_i64, _p, _p, _p, _p, _p, _i64, _p]),
    'chebgcn_metis_one_level_f64': (_i, [_i64, _p, _p, _p, _p, _p, _i64, _p]),
    'chebgcn_compute_perm_level': (_i, [_p, _i64, _p, _i64, _p]),
    'chebgcn_bank_order': (_i, [_i, _p, _p, _i, _p, _p]),
    'chebgcn_spectral_transform': (_i, [_p, _p, _p, _i, _i, _i, _p]),
    'chebgcn_spectral_mix_fwd': (_i, [_p, _p, _p, _i, _i, _i, _i, _p]),
    'chebgcn_spectral_mix_bwd_x': (_i, [_p, _p, _p, _i, _i, _i, _i, _p]),
    'chebgcn_spectral_mix_bwd_w': (_i, [_p, _p, _p, _i, _i, _i, _i, _p]),
    'chebgcn_spectral_spline_expand': (_i, [_p, _p, _p, _i, _i, _i, _p]),
    'chebgcn_spectral_spline_expand_bwd': (_i, [_p, _p, _p, _i, _i, _i, _p]),
    'chebgcn_saliency_supported': (_i, [_i]),
    'chebgcn_saliency_seed': (_i, [_p, _p, _i, _i, _i, _p, _p, _i, _i, _p]),
    'chebgcn_saliency_path': (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _p]),
    'chebgcn_saliency_reduce': (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _p, _p, _i, _p, _p]),
    'chebgcn_occlusion_supported': (_i, [_i]),
    'chebgcn_occlusion_rows': (_i, [_p, _p, _p, _p, _p, _i64, _i, _i, _i, _i, _i, _i, _p]),
    'chebgcn_occlusion_score': (_i, [_p, _i64, _i, _i, _i, _i, _p, _i, _p, _p, _p]),
    'chebgcn_occlusion_class_sums': (_i, [_p, _p, _i, _i, _i, _p, _p]),
    'chebgcn_shapley_supported': (_i, [_i]),
    'chebgcn_shapley_rows': (_i, [_p, _p, _p, _p, _p, _p, _i64, _i, _i, _i, _i, _i, _i, _i, _p]),
    'chebgcn_shapley_score': (_i, [_p, _i64, _i, _i, _i, _i, _i, _p, _i, _p, _p]),
    'chebgcn_shapley_reduce': (_i, [_p, _p, _i, _i, _i, _p, _p]),
    'chebgcn_gradcam_weights': (_i, [_p, _i, _i, _i, _p, _p]),
    'chebgcn_gradcam_map': (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _i, _p, _i64, _p]),
    'chebgcn_gather_windows': (_i, [_p, _i64, _p, _p, _p, _p, _p, _i, _i, _i, _p]),
    'chebgcn_gather_windows_mix': (_i, [_p, _i64, _p, _p, _i, _p, _p, _p, _p, _i, _i, _i, _p]),
    'chebgcn_window_stats_workspace': (C.c_size_t, [_i64, _i, _i]),
    'chebgcn_window_stats': (_i, [_p, _i64, _p, _i64, _p, _p, _p, _p, _i, _i, _p, C.c_size_t, _p]),
    'chebgcn_gather_windows_indexed': (_i, [_p, _i64, _p, _i64, _i, _i, _p, _p, _i64, _i, _p, _p, _p, _p, _i, _i, _i, _p]),
    'chebgcn_window_stats_indexed_workspace': (C.c_size_t, [_i64, _i, _i]),
    'chebgcn_window_stats_indexed': (_i, [_p, _i64, _p, _i64, _i, _i, _p, _p, _p, _p, _i, _i, _p, C.c_size_t, _p]),
    'chebgcn_window_drop': (_i, [_p, _p, _i, _i, _i, _i, C.c_uint32, C.c_uint32, _p, _p, _p, _f, _p]),
    'chebgcn_gather_windows_reflect': (_i, [_p, _i64, _p, _p, _p, _p, _p, _p, _i, _i, _i, _p]),
    'chebgcn_fc_fwd_dropout_supported': (_i, [_i, _i, _i, _i]),
    'chebgcn_fc_fwd_dropout_workspace': (C.c_size_t, [_i, _i, _i, _i]),
    'chebgcn_fc_fwd_dropout': (_i, [_p, _i64, _i64, _p, _p, _p, _p, C.c_size_t, _p, _i, _i, _i, _i, _i, C.c_uint32, _i, _i, C.c_uint32,
                               _f, _p]),
    'chebgcn_mc_reduce_supported': (_i, [_i, _i]),
    'chebgcn_mc_reduce': (_i, [_p, _i, _i, _i, _p, _p, _p, _p, _p, _p, _p, _p]),
    'chebgcn_knn_workspace': (C.c_size_t, [_i, _i, _i]),
    'chebgcn_knn': (_i, [_p, _i, _i, _i, _i, _p, _p, _p, C.c_size_t, _p]),
    'chebgcn_series_normalise': (_i, [_p, _i64, _p, _i, _i, _f, _p, _p]),
    'chebgcn_parcellate_query': (_i, [_i]),
    'chebgcn_parcellate': (_i, [_p, _i64, _p, _p, _i64, _p, _p, _i64, _i64, _i, _i, _i, _p]),
    'chebgcn_parcel_expand': (_i, [_p, _p, _p, _i64, _i, _i, _f, _p]),
    'chebgcn_cheb_filter_workspace': (C.c_size_t, [_p, _i, _i, _i, _i]),
    'chebgcn_cheb_filter': (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _i, _p]),
    'chebgcn_cluster_query': (_i, [_i]),
    'chebgcn_cluster_enhance_workspace': (C.c_size_t, [_i, _i, _i, _i]),
    'chebgcn_signflip_t': (_i, [_p, _p, _p, _p, _i, _i, C.c_uint32, _i, C.c_uint32, _p]),
    'chebgcn_perm_glm_query': (_i, [_i]),
    'chebgcn_perm_glm_t': (_i, [_p, _p, _p, _p, C.c_double, _i, _p, _p, _i, _i, _i, _i, _p]),
    'chebgcn_cluster_enhance': (_i, [_p, _p, _i64, _p, _i, _p, _p, _i, _p, C.c_double, _p, _p, _p, _p, _p, C.c_size_t, _i, _i, _i,
                                     _i, _p]),
    'chebgcn_glm_query': (_i, [_i]),
    'chebgcn_glm_workspace': (C.c_size_t, [_i, _i, _i]),
    'chebgcn_glm_project': (_i, [_p, _i64, _p, _i, _i, _p, _i, _p, _p, _p]),
    'chebgcn_glm_finish': (_i, [_p, _p, _p, _i64, _p, _p, _p, _p, _i, _i, _i, _i, _i, _p, _p, _p, _p, _p, _p, _p]),
    'chebgcn_glm_combine': (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _i, _p, _p, _p, _p]),
    'chebgcn_glm_ar1_query': (_i, [_i]),
    'chebgcn_glm_ar1_workspace': (C.c_size_t, [_i, _i, _i]),
    'chebgcn_glm_project_ar1': (_i, [_p, _i64, _p, _i, _i, _p, _i, _p, _p, _p, _p]),
    'chebgcn_glm_finish_ar1': (_i, [_p, _p, _p, _p, _p, _p, _i64, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, C.c_double,
                                    _p, _p, _p, _p, _p, _p, _p, _p]),
    'chebgcn_glm_trials_query': (_i, [_i]),
    'chebgcn_glm_trials': (_i, [_p, _i64, _p, _i, _i, _p, _i, _p, _p, _p, _i, _p, _p, _p, _p, _p, _i, _i64, _p, _p, _p, _p]),
    'chebgcn_searchlight_query': (_i, [_i]),
    'chebgcn_searchlight_spread': (_i, [_p, _i, _i, _p, _p, _i, _i, _p, _p]),
    'chebgcn_searchlight_fit': (_i, [_p, _i, _i, _p, _p, _i, _i, _i, _i, _p, _p, _p, _p]),
    'chebgcn_searchlight_score': (_i, [_p, _i, _i, _p, _p, _i, _i, _i, _i, _p, _i, _i, _i, _p, _p, _p, _p, _p, _p, _i, _p, _p, _p, _p,
                                       _p]),
    'chebgcn_searchlight_lda_query': (_i, [_i]),
    'chebgcn_searchlight_lda': (_i, [_p, _i, _i, _p, _p, _i, _i, _p, _i, _i, _p, _p, _i, _p, _i, _i, _i, _p, _p, C.c_double, _p, _p, _p, _i, _p,
                                     _p, _p, _p, _p]),
    'chebgcn_searchlight_rdm_query': (_i, [_i]),
    'chebgcn_searchlight_rdm': (_i, [_p, _i, _i, _p, _p, _i, _i, _p, _i, _i, _p, _p, _p, _i, _i, _i, _p, C.c_double, _i, _p, _p, _p]),
    'chebgcn_searchlight_svm_query': (_i, [_i]),
    'chebgcn_searchlight_svm': (_i, [_p, _i, _i, _p, _p, _i, _i, _p, _i, _p, _i, _i, _p, _p, _i, _p, _i, _i, _i, C.c_double, _i, C.c_double, _i,
                                     _p, _p, _p, _i, _p, _p, _p, _p, _p, _p]),
    'chebgcn_connectome_query': (_i, [_i]),
    'chebgcn_connectome_workspace': (C.c_size_t, [_i, _i]),
    'chebgcn_connectome_cov': (_i, [_p, _i64, _p, _i, _i, _p, C.c_size_t, _p]),
    'chebgcn_connectome_finish': (_i, [_p, C.c_size_t, _p, _i64, _i, _i, _i, C.c_double, _p, _p, _p, _p]),
    'chebgcn_connectome_mean': (_i, [_p, _p, _i, _i, _p, _p]),
    'chebgcn_connectome_sigma': (_i, [_p, C.c_size_t, _p, _i64, _i, _i, C.c_double, _p, _p, _p]),
    'chebgcn_tangent_query': (_i, [_i]),
    'chebgcn_tangent_workspace': (C.c_size_t, [_i, _i]),
    'chebgcn_sym_eigh': (_i, [_p, _i, _i, _p, _p, _p, _p, _p, C.c_size_t, _p]),
    'chebgcn_sym_function': (_i, [_p, _p, _i, _i, _i, C.c_double, _p, _i, _p, _p, _p]),
    'chebgcn_sym_congruence': (_i, [_p, _p, _i, _i, _p, _p, _p]),
    'chebgcn_sym_mean': (_i, [_p, _p, _i, _i, _i, _i, _p, _p, _p, _p]),
    'chebgcn_ridge_query': (_i, [_i]),
    'chebgcn_ridge_workspace': (C.c_size_t, [_i, _i, _i]),
    'chebgcn_ridge_rotate': (_i, [_p, _i, _p, _p, _i, _p, _i, _i, _i, _p, C.c_size_t, _p]),
    'chebgcn_ridge_score': (_i, [_p, C.c_size_t, _p, _i, _p, _p, _i, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _p, _p, _p, _p, _p]),
    'chebgcn_ridge_weights': (_i, [_p, C.c_size_t, _p, _p, _p, _p, _i, _i, _i, _i, _i, _p, _p]),
}

_lib = None


def lib():
    """The loaded library; raises ChebgcnError with build instructions if absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ChebgcnError(
                'libchebgcn.so not found at %s: build it with '
                '`python -c "import __graft_entry__ as g; g.build()"` or '
                '`make -C gcn_fmri_decoding_amd/csrc` (needs hipcc, --offload-arch=gfx950). '
                'There is no CPU fallback.' % LIB_PATH)
        # PyTorch first: libchebgcn.so needs libamdhip64, and the copy PyTorch bundles must be the one
        # in the process -- loaded the other way round, two HIP runtimes coexist and ours sees no device
        import torch  # noqa: F401
        handle = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(handle, name)        # AttributeError if the symbol is missing
            fn.restype = res
            fn.argtypes = args
        _lib = handle
    return _lib


# When a list: every checked launching call appends (what, chebgcn_last_dispatch()) -- the kernel templates the
# dispatchers chose for that call.  Tests assert the instantiation they claim to reach with it; None = off.
dispatch_log = None


def check(rc, what):
    if rc != 0:
        msg = lib().chebgcn_last_error()
        raise ChebgcnError('%s failed (%d): %s' % (what, rc, msg.decode() if msg else '?'))
    if dispatch_log is not None:
        dispatch_log.append((what, lib().chebgcn_last_dispatch().decode()))


def last_dispatch():
    """Kernel templates the calling thread's last launching entry point enqueued (chebgcn_last_dispatch)."""
    return lib().chebgcn_last_dispatch().decode()


def plane_stride(M):
    """Padded plane length; pure arithmetic, identical to chebgcn_plane_stride()."""
    return (int(M) + 31) & ~31
