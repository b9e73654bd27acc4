"""ctypes binding of libmvs_hip.so (include/mvs_hip.h).

The library is the product: if it is missing or cannot be loaded this module raises -- there is no
Python or CPU fallback for the hot path.
"""
import ctypes
import os
import weakref

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# MVS_HIP_LIBRARY: profiling tools point this at the ablation build (make -C csrc ablations); nothing else should
LIB_PATH = os.environ.get("MVS_HIP_LIBRARY") or os.path.join(_HERE, "libmvs_hip.so")

MVS_OK, MVS_E_INVALID, MVS_E_HIP, MVS_E_CAPACITY, MVS_E_NOMEM, MVS_E_RANGE, MVS_E_ABORTED, MVS_E_INTERNAL = 0, 1, 2, 3, 4, 5, 6, 7
MEM_HOST, MEM_DEVICE = 0, 1
KEEP_INT32, KEEP_INT16 = 0, 1
TOPK_EXCLUDE_SELF = 1
HDBSCAN_NO_ROOTS = 1
CONTAIN_ROW, CONTAIN_MAX = 0, 1
LIMBS_K3 = 0x103
MAX_GROUP_SLOTS = 16384
BLOCK_SYMMETRIC, BLOCK_MIRROR_ALL = 1, 2

CELL_DTYPE = np.dtype([("row", "<i4"), ("col", "<i4"), ("dot", "<i4"), ("q", "<i4")])
LINK_DTYPE = np.dtype([("a", "<i4"), ("b", "<i4"), ("dot", "<i4"), ("q", "<i4"), ("jaccard", "<f8")])      # mvs_link
HDBSCAN_CLUSTER_DTYPE = np.dtype([("parent", "<i4"), ("size", "<i4"), ("selected", "<i4"), ("representative", "<i4"), ("birth", "<i8"),
                                  ("death", "<i8"), ("stability", "<i8")])                                       # mvs_hdbscan_cluster
HMERGE_DTYPE = np.dtype([("a", "<i4"), ("b", "<i4"), ("round", "<i4"), ("size", "<i4"), ("sum", "<u8"), ("height", "<f8")])            # mvs_hmerge
HCLUST_METHODS = {"average": 0, "complete": 1}
HCLUST_MAX_TOTAL = 131072
GATHER_DTYPE = np.dtype([("sample", "<i4"), ("intersect", "<i4"), ("unique", "<i4"), ("remaining", "<i4")])  # mvs_gather_match
ABUND_OVERLAP_DTYPE = np.dtype([("inter", "<i8"), ("w_row", "<u8"), ("w_col", "<u8"), ("w_min", "<u8"), ("dot_lo", "<u8"),
                                ("dot_hi", "<u8")])                                                     # mvs_abund_overlap

# every symbol include/mvs_hip.h declares: (name, restype, argtypes)
_c = ctypes
_P = _c.c_void_p


class RowBlock(ctypes.Structure):
    """mvs_row_block: one CSR piece of the streamed comparison result"""
    _fields_ = [("row_begin", _c.c_int64), ("row_end", _c.c_int64), ("n_cells", _c.c_int64),
                ("row_ptr", _c.POINTER(_c.c_int64)), ("col", _c.POINTER(_c.c_int32)),
                ("q", _c.POINTER(_c.c_uint8)), ("q16", _c.POINTER(_c.c_uint16))]


ROW_BLOCK_CB = ctypes.CFUNCTYPE(_c.c_int, _P, _c.POINTER(RowBlock))


class EncodedRows(ctypes.Structure):
    """mvs_encoded_rows: one piece of the streamed comparison result with its rows encoded in the shard codec"""
    _fields_ = [("row_begin", _c.c_int64), ("row_end", _c.c_int64), ("n_cells", _c.c_int64), ("n_rows", _c.c_int64),
                ("rows", _c.POINTER(_c.c_uint32)), ("first_col", _c.POINTER(_c.c_uint32)),
                ("offset", _c.POINTER(_c.c_uint64)), ("jac_bytes", _c.POINTER(_c.c_uint32)),
                ("bytes", _c.POINTER(_c.c_uint8)), ("n_bytes", _c.c_int64)]


ENCODED_ROWS_CB = ctypes.CFUNCTYPE(_c.c_int, _P, _c.POINTER(EncodedRows))


class PermanovaResult(ctypes.Structure):
    """mvs_permanova_result"""
    _fields_ = [("f", _c.c_double), ("r2", _c.c_double), ("p_value", _c.c_double), ("ss_total", _c.c_double),
                ("ss_within", _c.c_double), ("ss_between", _c.c_double), ("df_between", _c.c_int64), ("df_within", _c.c_int64),
                ("samples", _c.c_int64), ("groups", _c.c_int64), ("permutations", _c.c_int64)]


class SilhouetteResult(ctypes.Structure):
    """mvs_silhouette_result"""
    _fields_ = [("mean", _c.c_double), ("negative", _c.c_int64), ("samples", _c.c_int64), ("labelled", _c.c_int64), ("groups", _c.c_int64)]


class CommunityResult(ctypes.Structure):
    """mvs_community_result"""
    _fields_ = [("n", _c.c_int64), ("edges", _c.c_int64), ("levels", _c.c_int64), ("communities", _c.c_int64), ("composed", _c.c_int64),
                ("rounds", _c.c_int64), ("total_weight", _c.c_uint64), ("qnum_hi", _c.c_uint64), ("qnum_lo", _c.c_uint64),
                ("g_fixed", _c.c_int64)]


class TsneParams(ctypes.Structure):
    """mvs_tsne_params"""
    _fields_ = [("perplexity", _c.c_double), ("exaggeration", _c.c_double), ("learning_rate", _c.c_double), ("neighbours", _c.c_int64),
                ("iterations", _c.c_int64), ("exaggeration_iters", _c.c_int64), ("init", _c.c_int64), ("seed", _c.c_uint64)]


class TsneResult(ctypes.Structure):
    """mvs_tsne_result"""
    _fields_ = [("n", _c.c_int64), ("neighbours", _c.c_int64), ("entries", _c.c_int64), ("beta_zero_rows", _c.c_int64),
                ("iterations", _c.c_int64), ("S", _c.c_uint64), ("learning_rate", _c.c_double), ("kl", _c.c_double)]


SYMBOLS = [
    ("mvs_version", _c.c_char_p, []),
    ("mvs_last_error", _c.c_char_p, []),
    ("mvs_device_count", _c.c_int, [_c.POINTER(_c.c_int)]),
    ("mvs_ctx_create", _c.c_int, [_c.c_int, _c.POINTER(_P)]),
    ("mvs_ctx_destroy", _c.c_int, [_P]),
    ("mvs_ctx_set_option", _c.c_int, [_P, _c.c_char_p, _c.c_int64]),
    ("mvs_ctx_get_option", _c.c_int, [_P, _c.c_char_p, _c.POINTER(_c.c_int64)]),
    ("mvs_ctx_set_stream", _c.c_int, [_P, _P]),
    ("mvs_ctx_use_own_stream", _c.c_int, [_P]),
    ("mvs_ctx_synchronize", _c.c_int, [_P]),
    ("mvs_ctx_set_timing", _c.c_int, [_P, _c.c_int]),
    ("mvs_ctx_kernel_ms", _c.c_int, [_P, _c.c_int, _c.POINTER(_c.c_float)]),
    ("mvs_ctx_pairwise_candidates", _c.c_int, [_P, _c.POINTER(_c.c_int64)]),
    ("mvs_comm_library", _c.c_int, [_c.c_char_p, _c.c_size_t, _c.POINTER(_c.c_int)]),
    ("mvs_ctx_pairwise_stats", _c.c_int, [_P, _c.POINTER(_c.c_int64), _c.POINTER(_c.c_int64), _c.POINTER(_c.c_int64)]),
    ("mvs_project_csr", _c.c_int, [_P, _P, _c.c_int, _P, _c.c_int64, _c.c_int, _P, _c.c_int]),
    ("mvs_project_csr_stats", _c.c_int, [_P, _P, _c.c_int, _P, _c.c_int64, _c.c_int, _P, _c.c_int, _P,
                                          _c.POINTER(_c.c_int64)]),
    ("mvs_project_plan", _c.c_int, [_P, _c.c_int64, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _P, _c.c_int64,
                                     _c.POINTER(_c.c_int64)]),
    ("mvs_ctx_project_stats", _c.c_int, [_P, _c.POINTER(_c.c_int64), _c.POINTER(_c.c_int64), _c.POINTER(_c.c_int),
                                          _c.POINTER(_c.c_int)]),
    ("mvs_ctx_derived_stats", _c.c_int, [_P] + [_c.POINTER(_c.c_int64)] * 5),
    ("mvs_sketch_sumsq", _c.c_int, [_P, _P, _c.c_int, _c.c_int64, _c.c_int, _P, _c.c_int]),
    ("mvs_sketch_stats", _c.c_int, [_P, _P, _c.c_int, _c.c_int64, _c.c_int, _P, _c.c_int, _c.POINTER(_c.c_int64)]),
    ("mvs_norms_sq_text", _c.c_int, [_P, _P, _c.c_int64, _c.c_int, _P]),
    ("mvs_sketch_saturate_i16", _c.c_int, [_P, _P, _c.c_int, _c.c_int64, _P, _c.c_int]),
    ("mvs_sketch_max_abs", _c.c_int, [_P, _P, _c.c_int, _c.c_int, _c.c_int64, _c.POINTER(_c.c_int64)]),
    ("mvs_limbs_for_max_abs", _c.c_int, [_c.c_int64]),
    ("mvs_limb_geometry", _c.c_int, [_c.c_int64, _c.c_int, _c.c_int, _c.POINTER(_c.c_int64),
                                      _c.POINTER(_c.c_int), _c.POINTER(_c.c_size_t)]),
    ("mvs_limb_split", _c.c_int, [_P, _P, _c.c_int, _c.c_int, _c.c_int64, _c.c_int, _c.c_int, _P, _c.c_int,
                                   _c.c_int64]),
    ("mvs_sketch_set_create", _c.c_int, [_P, _P, _c.c_int, _c.c_int, _c.c_int64, _c.c_int, _c.POINTER(_P)]),
    ("mvs_sketch_set_from_planes", _c.c_int, [_P, _P, _c.c_int64, _c.c_int64, _c.c_int, _c.c_int, _c.c_int,
                                               _c.POINTER(_P)]),
    ("mvs_sketch_set_alloc", _c.c_int, [_P, _c.c_int64, _c.c_int, _c.c_int, _c.POINTER(_P)]),
    ("mvs_sketch_set_fill", _c.c_int, [_P, _P, _c.c_int, _c.c_int, _c.c_int64, _c.c_int64]),
    ("mvs_sketch_set_fill_stats", _c.c_int, [_P, _P, _c.c_int, _c.c_int, _c.c_int64, _c.c_int64, _c.POINTER(_c.c_int64)]),
    ("mvs_sketch_set_info", _c.c_int, [_P, _c.POINTER(_c.c_int64), _c.POINTER(_c.c_int), _c.POINTER(_c.c_int),
                                        _c.POINTER(_c.c_int64), _c.POINTER(_c.c_int)]),
    ("mvs_sketch_set_destroy", _c.c_int, [_P]),
    ("mvs_pairwise_rows", _c.c_int, [_P, _P, _P, _c.c_int, _c.c_int, _c.c_int64, _c.c_int64, _P, _c.c_int64,
                                      _c.c_int, _c.POINTER(_c.c_int64)]),
    ("mvs_pairwise_stream", _c.c_int, [_P, _P, _P, _c.c_int, _c.c_int, _c.c_int64, _c.c_int64, _c.c_size_t, ROW_BLOCK_CB, _P,
                                        _c.POINTER(_c.c_int64)]),
    ("mvs_pairwise_stream_encoded", _c.c_int, [_P, _P, _P, _c.c_int, _c.c_int, _c.c_int64, _c.c_int64, _c.c_size_t,
                                                ENCODED_ROWS_CB, _P, _c.POINTER(_c.c_int64)]),
    ("mvs_ctx_stream_stats", _c.c_int, [_P, _c.POINTER(_c.c_double), _c.POINTER(_c.c_int64), _c.POINTER(_c.c_int64),
                                         _c.POINTER(_c.c_int64), _c.POINTER(_c.c_int)]),
    ("mvs_ctx_stream_dense_stats", _c.c_int, [_P] + [_c.POINTER(_c.c_int64)] * 4),
    ("mvs_pairwise_block", _c.c_int, [_P, _P, _P, _c.c_int, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int,
                                       _P, _c.c_int64, _c.POINTER(_c.c_int64)]),
    ("mvs_cells_sort", _c.c_int, [_P, _P, _c.c_int64, _P]),
    ("mvs_search_block", _c.c_int, [_P, _P, _P, _c.c_double, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int64, _P,
                                     _c.c_int64, _c.POINTER(_c.c_int64)]),
    ("mvs_pairwise_topk", _c.c_int, [_P, _P, _P, _c.c_int, _c.c_int, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int64,
                                      _c.c_int, _P, _c.c_int, _c.POINTER(_c.c_int64)]),
    ("mvs_ctx_topk_stats", _c.c_int, [_P, _c.POINTER(_c.c_double), _c.POINTER(_c.c_double), _c.POINTER(_c.c_int64),
                                       _c.POINTER(_c.c_int64)]),
    ("mvs_pairwise_contain", _c.c_int, [_P, _P, _P, _c.c_int, _c.c_double, _c.c_double, _c.c_int, _c.c_int64, _c.c_int64,
                                         _c.c_int64, _c.c_int64, _P, _c.c_int, _c.c_int64, _c.POINTER(_c.c_int64)]),
    ("mvs_ctx_contain_stats", _c.c_int, [_P, _c.POINTER(_c.c_double), _c.POINTER(_c.c_double), _c.POINTER(_c.c_int64),
                                          _c.POINTER(_c.c_int64)]),
    ("mvs_pairwise_levels", _c.c_int, [_P, _P, _P, _c.c_int, _P, _c.c_int, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int64, _P,
                                        _c.c_int, _P]),
    ("mvs_ctx_levels_stats", _c.c_int, [_P, _c.POINTER(_c.c_double), _c.POINTER(_c.c_double), _c.POINTER(_c.c_int64),
                                         _c.POINTER(_c.c_int64)]),
    ("mvs_sketch_moments", _c.c_int, [_P, _P, _c.c_int64, _c.c_int64, _P, _P, _c.c_int]),
    ("mvs_pca_fit", _c.c_int, [_P, _P, _c.c_int64, _c.c_int64, _c.c_int, _c.c_double, _c.c_int, _c.POINTER(_P)]),
    ("mvs_pca_info", _c.c_int, [_P, _c.POINTER(_c.c_int), _c.POINTER(_c.c_int), _c.POINTER(_c.c_int64), _c.POINTER(_c.c_int),
                                 _c.POINTER(_c.c_int), _c.POINTER(_c.c_double)]),
    ("mvs_pca_get", _c.c_int, [_P, _P, _P, _P, _P]),
    ("mvs_pca_transform", _c.c_int, [_P, _P, _P, _c.c_int64, _c.c_int64, _P, _c.c_int]),
    ("mvs_pca_destroy", _c.c_int, [_P]),
    ("mvs_ctx_pca_stats", _c.c_int, [_P, _c.POINTER(_c.c_double), _c.POINTER(_c.c_double), _c.POINTER(_c.c_double),
                                      _c.POINTER(_c.c_int64), _c.POINTER(_c.c_int64)]),
    ("mvs_jaccard_apply", _c.c_int, [_P, _P, _P, _c.c_int, _c.c_double, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int64, _P, _c.c_int,
                                      _c.c_int, _P, _c.c_int]),
    ("mvs_pcoa_fit", _c.c_int, [_P, _P, _P, _c.c_int, _c.c_int64, _c.c_int64, _c.c_int, _c.c_double, _c.c_double, _c.c_int,
                                 _c.POINTER(_P)]),
    ("mvs_pcoa_info", _c.c_int, [_P, _c.POINTER(_c.c_int64), _c.POINTER(_c.c_int64), _c.POINTER(_c.c_int), _c.POINTER(_c.c_int),
                                  _c.POINTER(_c.c_int), _c.POINTER(_c.c_int), _c.POINTER(_c.c_int), _c.POINTER(_c.c_double),
                                  _c.POINTER(_c.c_double), _c.POINTER(_c.c_double)]),
    ("mvs_pcoa_get", _c.c_int, [_P, _P, _P, _P, _P, _P]),
    ("mvs_pcoa_transform", _c.c_int, [_P, _P, _P, _P, _c.c_int, _c.c_int64, _c.c_int64, _P, _c.c_int]),
    ("mvs_pcoa_destroy", _c.c_int, [_P]),
    ("mvs_ctx_pcoa_stats", _c.c_int, [_P, _c.POINTER(_c.c_double), _c.POINTER(_c.c_double), _c.POINTER(_c.c_double),
                                       _c.POINTER(_c.c_int64), _c.POINTER(_c.c_int64), _c.POINTER(_c.c_int64)]),
    ("mvs_group_sums", _c.c_int, [_P, _P, _P, _c.c_int, _c.c_double, _c.c_int64, _c.c_int64, _P, _c.c_int64, _c.c_int, _P, _P, _P]),
    ("mvs_permutation_labels", _c.c_int, [_P, _c.c_int64, _c.c_int64, _c.c_uint64, _P]),
    ("mvs_permanova_stats", _c.c_int, [_P, _P, _P, _c.c_int64, _c.c_int, _c.c_int64, _c.POINTER(PermanovaResult), _P, _P]),
    ("mvs_permanova", _c.c_int, [_P, _P, _P, _c.c_int, _c.c_double, _c.c_int64, _c.c_int64, _P, _c.c_int, _c.c_int64, _c.c_uint64,
                                  _c.POINTER(PermanovaResult), _P, _P, _P]),
    ("mvs_ctx_groups_stats", _c.c_int, [_P, _c.POINTER(_c.c_double), _c.POINTER(_c.c_double), _c.POINTER(_c.c_double),
                                         _c.POINTER(_c.c_int64), _c.POINTER(_c.c_int64), _c.POINTER(_c.c_int64)]),
    ("mvs_label_sums", _c.c_int, [_P, _P, _P, _c.c_int, _c.c_double, _c.c_int64, _c.c_int64, _P, _c.c_int, _P, _P, _P, _P]),
    ("mvs_silhouette_stats", _c.c_int, [_P, _c.c_int64, _c.c_int, _P, _P, _P, _P, _c.POINTER(SilhouetteResult), _P, _P, _P, _P, _P, _P, _P, _P]),
    ("mvs_silhouette", _c.c_int, [_P, _P, _P, _c.c_int, _c.c_double, _c.c_int64, _c.c_int64, _P, _c.c_int, _c.POINTER(SilhouetteResult),
                                   _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    ("mvs_ctx_label_stats", _c.c_int, [_P, _c.POINTER(_c.c_double), _c.POINTER(_c.c_double), _c.POINTER(_c.c_double),
                                        _c.POINTER(_c.c_int64), _c.POINTER(_c.c_int64)]),
    ("mvs_hclust_sums", _c.c_int, [_P, _P, _c.c_int, _P, _c.c_int64, _c.c_int, _P, _c.POINTER(_c.c_int64)]),
    ("mvs_hclust_weights", _c.c_int, [_P, _P, _c.c_int, _c.c_int64, _c.c_int, _P, _c.POINTER(_c.c_int64)]),
    ("mvs_hclust", _c.c_int, [_P, _P, _P, _c.c_int, _c.c_double, _c.c_int64, _c.c_int64, _c.c_int, _P, _c.POINTER(_c.c_int64)]),
    ("mvs_hclust_order", _c.c_int, [_c.c_int64, _P, _P]),
    ("mvs_hclust_cut", _c.c_int, [_c.c_int64, _P, _c.c_double, _P]),
    ("mvs_hclust_cut_count", _c.c_int, [_c.c_int64, _P, _c.c_int64, _P]),
    ("mvs_ctx_hclust_stats", _c.c_int, [_P] + [_c.POINTER(_c.c_double)] * 5 + [_c.POINTER(_c.c_int64)] * 4),
    ("mvs_cluster_create", _c.c_int, [_P, _c.c_int64, _c.POINTER(_P)]),
    ("mvs_cluster_add_cells", _c.c_int, [_P, _P, _c.c_int64]),
    ("mvs_pairwise_cluster", _c.c_int, [_P, _P, _P, _c.c_int, _c.c_double, _P]),
    ("mvs_cluster_finish", _c.c_int, [_P, _P, _c.c_int, _P, _P, _P, _P, _c.c_int, _c.POINTER(_c.c_int64)]),
    ("mvs_cluster_destroy", _c.c_int, [_P]),
    ("mvs_ctx_cluster_stats", _c.c_int, [_P, _c.POINTER(_c.c_double), _c.POINTER(_c.c_double), _c.POINTER(_c.c_int64),
                                          _c.POINTER(_c.c_int64), _c.POINTER(_c.c_int64)]),
    ("mvs_linkage_create", _c.c_int, [_P, _c.c_int64, _c.c_int, _P, _c.c_int, _c.POINTER(_P)]),
    ("mvs_linkage_set_core", _c.c_int, [_P, _P, _c.c_int]),
    ("mvs_linkage_add_cells", _c.c_int, [_P, _P, _c.c_int64]),
    ("mvs_pairwise_linkage", _c.c_int, [_P, _P, _P, _c.c_int, _c.c_double, _P]),
    ("mvs_linkage_finish", _c.c_int, [_P, _P, _c.c_int64, _c.c_int, _c.POINTER(_c.c_int64)]),
    ("mvs_linkage_cells", _c.c_int, [_P, _c.c_double, _P, _c.c_int64, _c.POINTER(_c.c_int64)]),
    ("mvs_linkage_destroy", _c.c_int, [_P]),
    ("mvs_ctx_linkage_stats", _c.c_int, [_P, _c.POINTER(_c.c_double), _c.POINTER(_c.c_double), _c.POINTER(_c.c_int64),
                                          _c.POINTER(_c.c_int64), _c.POINTER(_c.c_int64)]),
    ("mvs_core_jaccard", _c.c_int, [_P, _P, _P, _c.c_int, _c.c_int, _P, _c.c_int]),
    ("mvs_hdbscan_select", _c.c_int, [_c.c_int64, _P, _c.c_int64, _P, _c.c_double, _c.c_int64, _c.c_int, _P, _P, _P, _P, _c.c_int64,
                                       _c.POINTER(_c.c_int64)]),
    ("mvs_hdbscan", _c.c_int, [_P, _P, _P, _c.c_int, _c.c_int, _c.c_double, _c.c_int64, _c.c_int, _P, _P, _c.POINTER(_c.c_int64), _P, _P, _P,
                                _P, _c.c_int64, _c.POINTER(_c.c_int64)]),
    ("mvs_ctx_hdbscan_stats", _c.c_int, [_P] + [_c.POINTER(_c.c_double)] * 6 + [_c.POINTER(_c.c_int64)] * 4),
    ("mvs_sketch_set_gather", _c.c_int, [_P, _P, _P, _c.c_int, _c.c_int64, _c.POINTER(_P)]),
    ("mvs_derep_create", _c.c_int, [_P, _c.c_int64, _c.POINTER(_P)]),
    ("mvs_derep_add_rows", _c.c_int, [_P, _P, _c.c_int64, _c.c_int64, _c.c_int64]),
    ("mvs_pairwise_derep", _c.c_int, [_P, _P, _P, _c.c_int, _c.c_double, _P]),
    ("mvs_derep_finish", _c.c_int, [_P, _P, _c.c_int, _P, _P, _P, _P, _c.c_int, _c.POINTER(_c.c_int64)]),
    ("mvs_derep_destroy", _c.c_int, [_P]),
    ("mvs_ctx_derep_stats", _c.c_int, [_P, _c.POINTER(_c.c_double), _c.POINTER(_c.c_double), _c.POINTER(_c.c_int64),
                                        _c.POINTER(_c.c_int64), _c.POINTER(_c.c_int64)]),
    ("mvs_dereplicate", _c.c_int, [_P, _P, _P, _c.c_int, _c.c_double, _P, _P, _P, _P, _P, _c.c_int, _c.POINTER(_c.c_int64)]),
    ("mvs_hash_set_create", _c.c_int, [_P, _P, _c.c_int, _P, _c.c_int64, _c.POINTER(_P)]),
    ("mvs_hash_set_info", _c.c_int, [_P, _c.POINTER(_c.c_int64), _c.POINTER(_c.c_int64), _c.POINTER(_c.c_int)]),
    ("mvs_hash_set_sizes", _c.c_int, [_P, _P, _c.c_int]),
    ("mvs_hash_set_destroy", _c.c_int, [_P]),
    ("mvs_kmer_max_hash", _c.c_int, [_c.c_int64, _c.POINTER(_c.c_uint64)]),
    ("mvs_kmer_hash", _c.c_int, [_c.c_char_p, _c.c_int, _c.c_uint32, _c.POINTER(_c.c_uint64), _c.POINTER(_c.c_int)]),
    ("mvs_hash_set_from_sequences", _c.c_int, [_P, _P, _c.c_int, _P, _c.c_int64, _c.c_int, _c.c_uint32, _c.c_uint64, _c.POINTER(_P)]),
    ("mvs_hash_set_export", _c.c_int, [_P, _P, _c.c_int, _P]),
    ("mvs_hash_set_device", _c.c_int, [_P, _c.POINTER(_P)]),
    ("mvs_ctx_kmer_stats", _c.c_int, [_P, _c.POINTER(_c.c_double)] + [_c.POINTER(_c.c_int64)] * 5),
    ("mvs_ctx_kmer_sample_stats", _c.c_int, [_P, _c.c_int64, _P, _P]),
    ("mvs_translate_codon", _c.c_int, [_c.c_char_p, _c.c_char_p, _c.POINTER(_c.c_int)]),
    ("mvs_aa_hash", _c.c_int, [_c.c_char_p, _c.c_int, _c.c_int, _c.c_uint32, _c.POINTER(_c.c_uint64), _c.POINTER(_c.c_int)]),
    ("mvs_hash_set_from_residues", _c.c_int, [_P, _P, _c.c_int, _P, _c.c_int64, _c.c_int, _c.c_int, _c.c_int, _c.c_uint32, _c.c_uint64, _c.POINTER(_P)]),
    ("mvs_ctx_aa_stats", _c.c_int, [_P, _c.POINTER(_c.c_double)] + [_c.POINTER(_c.c_int64)] * 5),
    ("mvs_ctx_aa_sample_stats", _c.c_int, [_P, _c.c_int64, _P, _P]),
    ("mvs_kmer_sketcher_create", _c.c_int, [_P, _c.c_int64, _c.c_int, _c.c_uint32, _c.c_uint64, _c.POINTER(_P)]),
    ("mvs_kmer_sketcher_add", _c.c_int, [_P, _P, _c.c_int, _P, _P, _c.c_int64]),
    ("mvs_kmer_sketcher_finish", _c.c_int, [_P, _c.c_uint32, _c.c_uint32, _P, _c.POINTER(_P)]),
    ("mvs_kmer_sketcher_stats", _c.c_int, [_P, _P, _P, _P, _P, _P]),
    ("mvs_kmer_sketcher_info", _c.c_int, [_P, _c.POINTER(_c.c_double)] + [_c.POINTER(_c.c_int64)] * 5),
    ("mvs_kmer_sketcher_destroy", _c.c_int, [_P]),
    ("mvs_hash_set_create_counted", _c.c_int, [_P, _P, _c.c_int, _P, _c.c_int, _P, _c.c_int64, _c.c_uint32, _c.c_uint32, _P, _c.POINTER(_P)]),
    ("mvs_hash_set_abundances", _c.c_int, [_P, _P, _c.c_int]),
    ("mvs_ctx_abund_stats", _c.c_int, [_P, _c.POINTER(_c.c_double), _c.POINTER(_c.c_double)] + [_c.POINTER(_c.c_int64)] * 5),
    ("mvs_intersect_cells", _c.c_int, [_P, _P, _P, _P, _c.c_int, _c.c_int64, _P, _c.c_int]),
    ("mvs_ctx_intersect_stats", _c.c_int, [_P, _c.POINTER(_c.c_double), _c.POINTER(_c.c_int64), _c.POINTER(_c.c_int64),
                                            _c.POINTER(_c.c_int64)]),
    ("mvs_abund_overlap_cells", _c.c_int, [_P, _P, _P, _P, _c.c_int, _c.c_int64, _P, _c.c_int]),
    ("mvs_hash_set_abundance_totals", _c.c_int, [_P, _P, _P, _P, _c.c_int]),
    ("mvs_abund_similarity", _c.c_int, [_P, _c.c_uint64, _c.c_uint64, _c.c_uint64, _c.c_int64, _c.c_uint64, _c.c_uint64, _c.c_uint64,
                                         _c.c_int64, _c.POINTER(_c.c_double)]),
    ("mvs_gather", _c.c_int, [_P, _P, _c.c_int64, _P, _P, _c.c_int, _c.c_int64, _c.c_int32, _c.c_int64, _P, _c.c_int,
                               _c.POINTER(_c.c_int64), _c.POINTER(_c.c_int32)]),
    ("mvs_ctx_gather_stats", _c.c_int, [_P, _c.POINTER(_c.c_int64), _c.POINTER(_c.c_int64), _c.POINTER(_c.c_int64),
                                         _c.POINTER(_c.c_int64), _c.POINTER(_c.c_double), _c.POINTER(_c.c_double),
                                         _c.POINTER(_c.c_double)]),
    ("mvs_ctx_gather_round_bytes", _c.c_int, [_P, _c.POINTER(_c.c_int64)]),
    ("mvs_pairwise_dots", _c.c_int, [_P, _P, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int64, _P, _c.c_int,
                                      _c.c_int]),
    ("mvs_sketch_set_planes", _c.c_int, [_P, _c.POINTER(_P)]),
    ("mvs_sketch_set_touch", _c.c_int, [_P]),
    ("mvs_comm_unique_id", _c.c_int, [_P]),
    ("mvs_comm_create", _c.c_int, [_P, _P, _c.c_int, _c.c_int, _c.POINTER(_P)]),
    ("mvs_comm_create_callbacks", _c.c_int, [_P, _P, _c.c_int, _c.c_int, _c.POINTER(_P)]),
    ("mvs_comm_create_files", _c.c_int, [_P, _c.c_char_p, _c.c_int, _c.c_int, _c.POINTER(_P)]),
    ("mvs_comm_create_rendezvous", _c.c_int, [_P, _c.c_char_p, _c.c_int, _c.c_int, _c.POINTER(_P)]),
    ("mvs_comm_destroy", _c.c_int, [_P]),
    ("mvs_comm_info", _c.c_int, [_P, _c.POINTER(_c.c_int), _c.POINTER(_c.c_int), _c.POINTER(_c.c_int)]),
    ("mvs_allgather_planes", _c.c_int, [_P, _P, _P, _c.c_int64, _c.c_int, _c.c_int]),
    ("mvs_allgather_rows", _c.c_int, [_P, _P, _P, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int, _c.c_int]),
    ("mvs_allgather_f64", _c.c_int, [_P, _P, _P, _c.c_int64]),
    ("mvs_allgather_bytes", _c.c_int, [_P, _P, _P, _c.c_int64]),
    ("mvs_allreduce_max_i64", _c.c_int, [_P, _P, _c.POINTER(_c.c_int64)]),
    ("mvs_shard_layout", _c.c_int, [_c.c_int64, _c.c_int, _c.POINTER(_c.c_int64), _c.POINTER(_c.c_int64)]),
    ("mvs_sketch_set_attach_derived", _c.c_int, [_P, _P, _P]),
    ("mvs_sketch_set_prepare_rows", _c.c_int, [_P, _P, _c.c_int64, _c.c_int64]),
    ("mvs_sketch_set_recode_rows", _c.c_int, [_P, _P, _P, _c.c_int, _c.c_int64, _c.c_int64, _c.c_int64]),
    ("mvs_sketch_set_planes_from_wire", _c.c_int, [_P, _P, _P, _c.c_int64, _c.c_int64]),
    ("mvs_plan_begin", _c.c_int, [_P, _P, _P, _c.c_int, _c.c_int64, _c.c_int64, _c.c_int, _P, _c.c_int64]),
    ("mvs_plan_wire", _c.c_int, [_P, _P]),
    ("mvs_plan_rows_ready", _c.c_int, [_P, _c.c_int64, _c.c_int64]),
    ("mvs_plan_filter", _c.c_int, [_P, _P, _c.c_int]),
    ("mvs_plan_finish", _c.c_int, [_P, _c.POINTER(_P)]),
    ("mvs_plan_stats", _c.c_int, [_P, _c.POINTER(_c.c_double), _c.POINTER(_c.c_int64)]),
    ("mvs_cells_route", _c.c_int, [_P, _P, _P, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int64, _P,
                                    _c.c_int64, _P, _P, _c.c_int64, _c.c_int64, _c.c_int64]),
    ("mvs_cells_collect", _c.c_int, [_P, _P, _c.c_int, _c.c_int, _c.c_int64, _c.c_int64, _c.c_int64, _P, _c.c_int64, _P]),
    ("mvs_cells_report", _c.c_int, [_P, _P, _c.c_int, _c.c_int64, _c.c_int64, _P, _c.POINTER(_c.c_int64)]),
    ("mvs_cells_sort_rows", _c.c_int, [_P, _P, _c.c_int64, _c.c_int64, _c.c_int64, _P, _P]),
    ("mvs_cells_sort_rows_ahead", _c.c_int, [_P, _P, _c.c_int64, _c.c_int64, _c.c_int64, _P, _P, _c.c_int64]),
    ("mvs_sketch_set_wire_rows", _c.c_int, [_P, _P, _P, _c.c_int64, _c.c_int64]),
    ("mvs_device_alloc", _c.c_int, [_P, _c.c_size_t, _c.c_int, _c.POINTER(_P)]),
    ("mvs_device_free", _c.c_int, [_P, _P]),
    ("mvs_device_zero", _c.c_int, [_P, _P, _c.c_size_t]),
    ("mvs_device_copy", _c.c_int, [_P, _P, _c.c_int, _P, _c.c_int, _c.c_size_t]),
    ("mvs_event_create", _c.c_int, [_P, _c.c_int, _c.POINTER(_P)]),
    ("mvs_event_record", _c.c_int, [_P, _P]),
    ("mvs_ctx_wait_event", _c.c_int, [_P, _P]),
    ("mvs_event_synchronize", _c.c_int, [_P]),
    ("mvs_event_elapsed_ms", _c.c_int, [_P, _P, _c.POINTER(_c.c_float)]),
    ("mvs_event_destroy", _c.c_int, [_P]),
    ("mvs_cells_stream", _c.c_int, [_P, _P, _c.c_int64, _c.c_int64, _c.c_int64, ROW_BLOCK_CB, _P, _c.POINTER(_c.c_int64)]),
    ("mvs_cells_stream_encoded", _c.c_int, [_P, _P, _c.c_int64, _c.c_int64, _c.c_int64, ENCODED_ROWS_CB, _P, _c.POINTER(_c.c_int64)]),
    ("mvs_community_create", _c.c_int, [_P, _c.c_int64, _c.c_int, _P, _c.c_int, _c.c_double, _c.POINTER(_P)]),
    ("mvs_community_add_cells", _c.c_int, [_P, _P, _c.c_int64]),
    ("mvs_community_add_edges", _c.c_int, [_P, _P, _P, _P, _c.c_int64, _c.c_int]),
    ("mvs_pairwise_community", _c.c_int, [_P, _P, _P, _c.c_int, _c.c_double, _P]),
    ("mvs_community_finish", _c.c_int, [_P, _c.c_double, _c.c_int64, _P, _P, _c.c_int64, _P, _P, _P, _P, _c.c_int, _P, _P, _P, _P,
                                         _c.POINTER(CommunityResult)]),
    ("mvs_community_destroy", _c.c_int, [_P]),
    ("mvs_communities", _c.c_int, [_P, _P, _P, _c.c_int, _c.c_double, _c.c_double, _c.c_int64, _P, _P, _c.c_int64, _P, _P, _P, _P,
                                    _c.c_int, _P, _P, _P, _P, _c.POINTER(CommunityResult)]),
    ("mvs_community_modularity", _c.c_int, [_c.c_int64, _P, _P, _P, _c.c_int64, _P, _c.c_int64, _c.POINTER(_c.c_uint64),
                                             _c.POINTER(_c.c_uint64)]),
    ("mvs_ctx_community_stats", _c.c_int, [_P] + [_c.POINTER(_c.c_double)] * 5 + [_c.POINTER(_c.c_int64)] * 6 + [_P]),
    ("mvs_tsne_create", _c.c_int, [_P, _c.c_int64, _c.POINTER(_P)]),
    ("mvs_tsne_destroy", _c.c_int, [_P]),
    ("mvs_tsne_add_edges", _c.c_int, [_P, _P, _P, _P, _c.c_int64, _c.c_int]),
    ("mvs_tsne_add_neighbours", _c.c_int, [_P, _P, _c.c_int64, _c.c_int, _P, _c.c_int, _c.c_int, _c.c_double, _P, _P]),
    ("mvs_tsne_finish_graph", _c.c_int, [_P]),
    ("mvs_tsne_edges", _c.c_int, [_P, _P, _P, _P, _c.c_int64, _c.POINTER(_c.c_int64), _c.POINTER(_c.c_uint64)]),
    ("mvs_tsne_set_state", _c.c_int, [_P, _P, _P, _P]),
    ("mvs_tsne_get_state", _c.c_int, [_P, _P, _P, _P]),
    ("mvs_tsne_gradient", _c.c_int, [_P, _c.c_double, _P, _P, _c.POINTER(_c.c_int64)]),
    ("mvs_tsne_run", _c.c_int, [_P, _c.c_int64, _c.c_double, _c.c_double, _c.c_double]),
    ("mvs_tsne_kl", _c.c_int, [_P, _c.POINTER(_c.c_double)]),
    ("mvs_tsne", _c.c_int, [_P, _P, _P, _c.c_int, _c.POINTER(TsneParams), _P, _P, _P, _c.POINTER(TsneResult), _c.POINTER(_P)]),
    ("mvs_ctx_tsne_stats", _c.c_int, [_P] + [_c.POINTER(_c.c_double)] * 6 + [_c.POINTER(_c.c_int64)] * 4),
    ("mvs_chunk_size", _c.c_int64, [_c.c_double, _c.c_int]),
    ("mvs_shard_rows", None, [_c.c_int64, _c.c_int, _c.c_int, _c.POINTER(_c.c_int64), _c.POINTER(_c.c_int64)]),
]

_lib = None


class MvsError(RuntimeError):
    def __init__(self, code, message, needed=None):
        super().__init__("libmvs_hip error %d: %s" % (code, message))
        self.code = code
        self.needed = needed     # MVS_E_CAPACITY: the size the call reported it needs


def load_library():
    """Load libmvs_hip.so (once).  torch, when present, is imported first so that the process uses a
    single HIP runtime (torch's bundled libamdhip64 has the same SONAME as the system one)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "libmvs_hip.so not found at %s -- build it with `make -C metagenome_vector_sketches_amd/csrc` "
            "(or __graft_entry__.build()); there is no CPU fallback" % LIB_PATH)
    try:
        import torch  # noqa: F401  (side effect: loads the HIP runtime torch ships)
    except Exception:  # torch is plumbing for tests/bench, not a requirement of the library
        pass
    lib = ctypes.CDLL(LIB_PATH)
    for name, restype, argtypes in SYMBOLS:
        fn = getattr(lib, name)  # AttributeError if the ABI is incomplete
        fn.restype = restype
        fn.argtypes = argtypes
    _lib = lib
    return lib


def _check(rc):
    if rc != MVS_OK:
        raise MvsError(rc, load_library().mvs_last_error().decode("utf-8", "replace"))


def _is_torch(x):
    return type(x).__module__.startswith("torch")


def _buf(x, dtype=None, writable=False):
    """-> (pointer, mem flag, keepalive).  numpy arrays are host buffers, torch CUDA tensors device."""
    if x is None:
        return None, MEM_HOST, None
    if isinstance(x, DeviceArray):
        return x.ptr, MEM_DEVICE, x
    if _is_torch(x):
        if not x.is_contiguous():
            raise ValueError("tensor must be contiguous")
        return x.data_ptr(), (MEM_DEVICE if x.is_cuda else MEM_HOST), x
    a = np.ascontiguousarray(x, dtype=dtype) if not writable else x
    if writable and (not a.flags["C_CONTIGUOUS"] or (dtype is not None and a.dtype != np.dtype(dtype))):
        raise ValueError("output array must be C-contiguous %s" % dtype)
    return a.ctypes.data, MEM_HOST, a


class DeviceArray:
    """`count` values of `dtype` at the device address `ptr`, owned by `owner` (which this object keeps alive): what
    HashSet.device_hashes returns, accepted wherever a device buffer of hashes is (Context.project_csr, Context.hash_set)."""

    def __init__(self, ptr, count, dtype, owner):
        self.ptr, self.count, self.dtype, self.owner = ptr, int(count), np.dtype(dtype), owner

    def __len__(self):
        return self.count


ABUND_MEASURES = ("w_contain_row", "w_contain_col", "bray_curtis", "ruzicka", "cosine", "angular")


def abund_similarity(overlap, totals_row, size_row, totals_col, size_col):
    """mvs_abund_similarity, pure host: the six measures of ABUND_MEASURES, in that order, as a float64 array.  overlap: one
    ABUND_OVERLAP_DTYPE record or a sequence (inter, w_row, w_col, w_min, dot_lo, dot_hi); totals_*: (sum, sumsq_lo, sumsq_hi)
    of the row / column sample, size_*: its number of values.  Needs no device."""
    rec = np.zeros(1, dtype=ABUND_OVERLAP_DTYPE)
    rec[0] = tuple(int(overlap[f]) for f in ABUND_OVERLAP_DTYPE.names) if hasattr(overlap, "dtype") and overlap.dtype == ABUND_OVERLAP_DTYPE \
        else tuple(int(v) for v in overlap)
    out = (_c.c_double * 6)()
    _check(load_library().mvs_abund_similarity(rec.ctypes.data, *[int(v) for v in totals_row], int(size_row),
                                               *[int(v) for v in totals_col], int(size_col), out))
    return np.array(out[:], dtype=np.float64)


def kmer_max_hash(scaled):
    """mvs_kmer_max_hash: the largest hash a FracMinHash sketch of this `scaled` keeps (scaled = 1: 2^64 - 1)"""
    out = _c.c_uint64()
    _check(load_library().mvs_kmer_max_hash(int(scaled), ctypes.byref(out)))
    return out.value


def kmer_hash(kmer, seed=42):
    """mvs_kmer_hash: the hash of one k-mer (bytes or str, 1 .. 32 letters) under the sketching rule -- canonical form,
    MurmurHash3_x64_128's first word --, or None if one of its bytes is not a base"""
    if isinstance(kmer, str):
        kmer = kmer.encode("latin-1")
    kmer = bytes(kmer)
    h, valid = _c.c_uint64(), _c.c_int()
    _check(load_library().mvs_kmer_hash(kmer, len(kmer), int(seed) & 0xFFFFFFFF, ctypes.byref(h), ctypes.byref(valid)))
    return h.value if valid.value else None


SEQ_PROTEIN, SEQ_TRANSLATE = 0, 1                                      # MVS_SEQ_*
AA_ALPHABETS = {"protein": 0, "dayhoff": 1, "hp": 2}                   # MVS_AA_*
AA_KSIZE = {"protein": 10, "dayhoff": 16, "hp": 42}                    # the customary ksize of each alphabet


def _alphabet(alphabet):
    if alphabet not in AA_ALPHABETS:
        raise ValueError("alphabet must be one of %s" % ", ".join(AA_ALPHABETS))
    return AA_ALPHABETS[alphabet]


def aa_hash(kmer, alphabet="protein", seed=42):
    """mvs_aa_hash: the hash of one protein k-mer (bytes or str, 1 .. 64 residues) in `alphabet` ("protein", "dayhoff", "hp") --
    MurmurHash3_x64_128's first word of the encoded residues --, or None if one of its bytes is not a residue"""
    if isinstance(kmer, str):
        kmer = kmer.encode("latin-1")
    kmer = bytes(kmer)
    h, valid = _c.c_uint64(), _c.c_int()
    _check(load_library().mvs_aa_hash(kmer, len(kmer), _alphabet(alphabet), int(seed) & 0xFFFFFFFF, ctypes.byref(h), ctypes.byref(valid)))
    return h.value if valid.value else None


def translate_codon(codon):
    """mvs_translate_codon: the residue (a one-letter str, '*' for a stop) of a codon of three bases (bytes or str) under the
    standard genetic code, or None if one of its bytes is not a base"""
    if isinstance(codon, str):
        codon = codon.encode("latin-1")
    codon = bytes(codon)
    if len(codon) != 3:
        raise ValueError("a codon is three bytes")
    aa, valid = _c.create_string_buffer(1), _c.c_int()
    _check(load_library().mvs_translate_codon(codon, aa, ctypes.byref(valid)))
    return aa.raw.decode("latin-1") if valid.value else None


def _norms(norms_sq):
    """_buf of n squared norms: a torch tensor as it is (host or device), anything else as a float64 array"""
    return _buf(norms_sq) if _is_torch(norms_sq) else _buf(norms_sq, np.float64)


def _cell_list(cells, n_cells):
    """-> (device pointer, n_cells, keepalive) of a device cell list: a torch CUDA tensor (int32 [m, 4]; the first n_cells
    rows, default all) or a device address (int) with n_cells"""
    if _is_torch(cells):
        cp, cm, ck = _buf(cells)
        if cm != MEM_DEVICE:
            raise ValueError("cells must be a device buffer")
        if n_cells is None:
            n_cells = cells.shape[0]
        elif n_cells > cells.shape[0]:
            raise ValueError("n_cells beyond the tensor")
        return cp, int(n_cells), ck
    if n_cells is None:
        raise ValueError("a raw device pointer needs n_cells")
    return (_P(int(cells)) if int(cells) else None), int(n_cells), None


class _Handle:
    """An object of the library held through its handle `_h` on the context `ctx`: close() destroys it once, through the
    library function `_destroy` names; a context manager; closed when collected."""
    _destroy = None

    def close(self):
        if self._h:
            getattr(self.ctx.lib, self._destroy)(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _Pieces:
    """What the streaming calls share: a ctypes callback that copies every piece out of the library's pinned buffer (an
    exception inside it must not unwind through the C frames: it is kept and raised after the call)."""

    def __init__(self, cb_type):
        self.parts, self.errors = [], []
        self.cb = cb_type(self._trampoline)

    def _trampoline(self, _user, bp):
        try:
            return self.take(bp.contents)
        except BaseException as e:      # noqa: BLE001
            self.errors.append(e)
            return -1

    def check(self, rc):
        if self.errors:
            raise self.errors[0]
        _check(rc)


class _RowBlockPieces(_Pieces):
    """CSR pieces (mvs_row_block) of mvs_pairwise_stream / mvs_cells_stream"""

    def __init__(self, on_block):
        super().__init__(ROW_BLOCK_CB)
        self.on_block = on_block

    def take(self, b):
        rows, n = b.row_end - b.row_begin, b.n_cells
        rp = np.ctypeslib.as_array(b.row_ptr, shape=(rows + 1,)).copy()
        col = np.ctypeslib.as_array(b.col, shape=(n,)).copy() if n else np.empty(0, np.int32)
        if n == 0:
            q = np.empty(0, np.uint8)
        elif b.q:
            q = np.ctypeslib.as_array(b.q, shape=(n,)).copy()
        else:
            q = np.ctypeslib.as_array(b.q16, shape=(n,)).copy()
        if self.on_block is not None:
            return 1 if self.on_block(b.row_begin, b.row_end, rp, col, q) else 0
        self.parts.append((b.row_begin, b.row_end, rp, col, q))
        return 0

    def join(self, row_begin, row_end, count):
        parts = self.parts
        rows = row_end - row_begin
        row_ptr = np.zeros(rows + 1, dtype=np.int64)
        at, expect = 0, row_begin
        for (b0, b1, rp, col, q) in parts:
            assert b0 == expect and rp[0] == 0, "pieces must arrive in ascending row order, each row once"
            row_ptr[b0 - row_begin:b1 - row_begin + 1] = rp + at
            at += int(rp[-1])
            expect = b1
        assert expect == row_end and at == count
        wide = any(p[4].dtype == np.uint16 for p in parts)
        col = np.concatenate([p[3] for p in parts]) if parts else np.empty(0, np.int32)
        q = np.concatenate([p[4].astype(np.uint16 if wide else np.uint8) for p in parts]) if parts else np.empty(0, np.uint8)
        return {"row_ptr": row_ptr, "col": col, "q": None if wide else q, "q16": q if wide else None, "n_cells": count,
                "pieces": len(parts)}


class _EncodedPieces(_Pieces):
    """pieces of finished shard records (mvs_encoded_rows) of mvs_pairwise_stream_encoded / mvs_cells_stream_encoded"""

    def __init__(self):
        super().__init__(ENCODED_ROWS_CB)

    def take(self, b):
        r, nb = b.n_rows, b.n_bytes

        def arr(ptr, n, dt):
            return np.ctypeslib.as_array(ptr, shape=(n,)).copy() if n else np.empty(0, dt)
        self.parts.append((b.row_begin, b.row_end, arr(b.rows, r, np.uint32), arr(b.first_col, r, np.uint32),
                           arr(b.offset, r, np.uint64), arr(b.jac_bytes, r, np.uint32), arr(b.bytes, nb, np.uint8), b.n_cells))
        return 0

    def join(self, row_begin, row_end, count):
        parts = self.parts
        expect, at = row_begin, 0
        offs = []
        for p in parts:
            assert p[0] == expect, "pieces must arrive in ascending row order"
            expect = p[1]
            offs.append(p[4] + np.uint64(at))
            at += len(p[6])
        assert expect == row_end and sum(p[7] for p in parts) == count
        cat = lambda i, dt: np.concatenate([p[i] for p in parts]) if parts else np.empty(0, dt)   # noqa: E731
        return {"rows": cat(2, np.uint32), "first_col": cat(3, np.uint32),
                "offset": np.concatenate(offs) if offs else np.empty(0, np.uint64), "jac_bytes": cat(5, np.uint32),
                "bytes": cat(6, np.uint8), "n_cells": count, "pieces": len(parts)}


class SketchSet(_Handle):
    """Limb planes of N samples resident in HBM (mvs_sketch_set)."""
    _destroy = "mvs_sketch_set_destroy"

    def __init__(self, ctx, handle, keep=None):
        self.ctx, self._h, self._keep = ctx, handle, keep
        ctx._sets.add(self)
        n, d, limbs, n_alloc, d_pad = (_c.c_int64(), _c.c_int(), _c.c_int(), _c.c_int64(), _c.c_int())
        _check(ctx.lib.mvs_sketch_set_info(handle, n, d, limbs, n_alloc, d_pad))
        self.n, self.d, self.limbs, self.n_alloc, self.d_pad = n.value, d.value, limbs.value, n_alloc.value, d_pad.value

    def fill(self, sketches, row_offset=0):
        """re-code `sketches` into rows [row_offset, row_offset + len) of a set made by sketch_set_alloc"""
        n, d = sketches.shape
        p, m, k = _buf(sketches)
        eb = self.ctx._elem_bytes(sketches)
        _check(self.ctx.lib.mvs_sketch_set_fill(self._h, p, eb, m, int(row_offset), n))

    def fill_stats(self, sketches, row_offset=0):
        """fill() that also returns the largest |v| of the rows it re-coded (one upload instead of a max_abs pass and a
        fill pass; a value beyond what the set's limb count holds means: allocate again with more limbs)"""
        n, d = sketches.shape
        p, m, k = _buf(sketches)
        eb = self.ctx._elem_bytes(sketches)
        mx = _c.c_int64()
        _check(self.ctx.lib.mvs_sketch_set_fill_stats(self._h, p, eb, m, int(row_offset), n, ctypes.byref(mx)))
        return mx.value

    def gather(self, rows):
        """-> a new SketchSet whose row i is row rows[i] of this one (mvs_sketch_set_gather): same d and limb code, rows may
        repeat; rows: int32 indices, numpy or a torch tensor (host or device).  A row outside [0, n) raises MVS_E_RANGE."""
        rp, rm, rk = _buf(rows) if _is_torch(rows) else _buf(rows, np.int32)
        if _is_torch(rows) and str(rows.dtype) != "torch.int32":
            raise ValueError("rows must be int32")
        h = _P()
        _check(self.ctx.lib.mvs_sketch_set_gather(self.ctx._h, self._h, rp, rm, len(rows), ctypes.byref(h)))
        return SketchSet(self.ctx, h)

    def touch(self):
        """the caller has rewritten the planes: data the library derived from them is rebuilt on the next comparison"""
        _check(self.ctx.lib.mvs_sketch_set_touch(self._h))


class ClusterResult:
    """What Cluster.finish / Context.cluster return: numpy int32 arrays `labels` (cluster of every sample; clusters numbered
    by ascending smallest member), `degree` (linked samples per sample), `representatives` and `sizes` (per cluster), and
    `n_clusters`."""

    def __init__(self, labels, degree, representatives, sizes):
        self.labels, self.degree, self.representatives, self.sizes = labels, degree, representatives, sizes
        self.n_clusters = len(sizes)

    def __repr__(self):
        return "ClusterResult(%d samples, %d clusters, largest %d)" % (
            len(self.labels), self.n_clusters, int(self.sizes.max()) if self.n_clusters else 0)


class Cluster(_Handle):
    """Single-linkage clusters of n samples, built on the device from lists of cells (mvs_cluster): every cell (row, col)
    says "these two belong together".  Feed it with add_cells (any device list: the output of Context.search_block /
    pairwise_block, a torch int32 tensor [m, 4] or a raw device pointer) or Context.cluster_into, read it with finish."""
    _destroy = "mvs_cluster_destroy"

    def __init__(self, ctx, n):
        self.ctx, self.n = ctx, int(n)
        h = _P()
        _check(ctx.lib.mvs_cluster_create(ctx._h, self.n, ctypes.byref(h)))
        self._h = h
        ctx._children.add(self)

    def add_cells(self, cells, n_cells=None):
        """cells: torch CUDA tensor (int32 [m, 4]; the first n_cells rows, default all) or a device address (int) with n_cells.
        degree[row] grows by one per cell with row != col: feeding a list twice changes `degree`, nothing else."""
        cp, n_cells, ck = _cell_list(cells, n_cells)
        _check(self.ctx.lib.mvs_cluster_add_cells(self._h, cp, n_cells))

    def finish(self, norms_sq):
        """-> ClusterResult; norms_sq (n doubles, numpy or torch) decides the representatives"""
        np_, nm, nk = _norms(norms_sq)
        n = self.n
        labels, degree = np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int32)
        reps, sizes = np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int32)
        count = _c.c_int64()
        _check(self.ctx.lib.mvs_cluster_finish(self._h, np_, nm, labels.ctypes.data, degree.ctypes.data, reps.ctypes.data,
                                               sizes.ctypes.data, MEM_HOST, ctypes.byref(count)))
        return ClusterResult(labels, degree, reps[:count.value].copy(), sizes[:count.value].copy())


COMMUNITY_MAX_LEVELS = 64
COMMUNITY_R = 1 << 12


def _i128(hi, lo):
    """hi * 2^64 + lo in two's complement -> Python int"""
    v = (int(hi) << 64) | int(lo)
    return v - (1 << 128) if v >> 127 else v


class Communities:
    """What CommunityGraph.finish / Context.communities return.  `labels` (int32 [n]: the community of every sample, numbered by
    smallest member), `level_labels` (int32 [levels, n]: the membership after every level, before the connected split), `qnum`
    (the final Qnum, a Python int) and `modularity` = qnum / (R W^2), `level_qnum` / `level_modularity` / `rounds` /
    `level_communities` per level, `sizes`, `internal` (in(C)) and `total` (tot(C)) per final community, `degree` and `strength`
    per sample, `edges`, `total_weight` (W), `composed` (communities before the split), `g_fixed`."""

    def __init__(self, res, labels, level_labels, degree, strength, internal, total, level_communities, rounds, level_qnum):
        self.labels, self.level_labels, self.degree, self.strength = labels, level_labels, degree, strength
        self.internal, self.total = internal, total
        self.level_communities, self.rounds, self.level_qnum = level_communities, rounds, level_qnum
        self.edges, self.total_weight, self.levels = int(res.edges), int(res.total_weight), int(res.levels)
        self.composed, self.g_fixed = int(res.composed), int(res.g_fixed)
        self.qnum = _i128(res.qnum_hi, res.qnum_lo)
        self.sizes = np.bincount(labels, minlength=int(res.communities)).astype(np.int64)
        self.n_communities = int(res.communities)

    def _mod(self, q):
        w = float(self.total_weight)
        return float(q) / (float(COMMUNITY_R) * w * w) if self.total_weight else 0.0

    @property
    def modularity(self):
        return self._mod(self.qnum)

    @property
    def level_modularity(self):
        return [self._mod(q) for q in self.level_qnum]

    def __repr__(self):
        return "Communities(%d samples, %d edges, %d communities, modularity %.4f, %d levels)" % (
            len(self.labels), self.edges, self.n_communities, self.modularity, self.levels)


class CommunityGraph(_Handle):
    """The thresholded Jaccard graph of n samples on the device and its modularity communities (mvs_community): feed it with
    add_cells (a device cell list; needs norms_sq and d), add_edges (raw integer edges lo, hi, a with 1 <= a <= 2^20) or
    Context.communities_into, read it with finish -- as often as wanted, at any resolution."""
    _destroy = "mvs_community_destroy"

    def __init__(self, ctx, n, d=0, norms_sq=None, floor=0.05):
        self.ctx, self.n = ctx, int(n)
        np_, nm, nk = _norms(norms_sq) if norms_sq is not None else (None, MEM_HOST, None)
        h = _P()
        _check(ctx.lib.mvs_community_create(ctx._h, self.n, int(d), np_, nm, float(floor), ctypes.byref(h)))
        self._h = h
        ctx._children.add(self)

    def add_cells(self, cells, n_cells=None):
        """cells: torch CUDA tensor (int32 [m, 4]; the first n_cells rows, default all) or a device address (int) with n_cells"""
        cp, n_cells, ck = _cell_list(cells, n_cells)
        _check(self.ctx.lib.mvs_community_add_cells(self._h, cp, n_cells))

    def add_edges(self, lo, hi, a):
        """raw edges: three int32 arrays of one length (numpy, or torch tensors that all live in the same place)"""
        if _is_torch(lo):
            (lp, lm, lk), (hp, hm, hk), (ap, am, ak) = _buf(lo), _buf(hi), _buf(a)
            if not (lm == hm == am):
                raise ValueError("lo, hi and a must live in the same place")
        else:
            (lp, lm, lk), (hp, hm, hk), (ap, am, ak) = _buf(lo, np.int32), _buf(hi, np.int32), _buf(a, np.int32)
        if not (len(lo) == len(hi) == len(a)):
            raise ValueError("lo, hi and a must have one length")
        _check(self.ctx.lib.mvs_community_add_edges(self._h, lp, hp, ap, len(lo), lm))

    def finish(self, resolution=1.0, max_rounds=100):
        """-> Communities"""
        return _communities_call(self.n, lambda *out: self.ctx.lib.mvs_community_finish(self._h, float(resolution), int(max_rounds), *out))


def _communities_call(n, call):
    """the outputs that mvs_community_finish and mvs_communities share"""
    cap = COMMUNITY_MAX_LEVELS
    labels, degree = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    level_labels = np.zeros((cap, n), dtype=np.int32)
    strength, internal, total = (np.zeros(n, dtype=np.uint64) for _ in range(3))
    lc, lr = np.zeros(cap, dtype=np.int64), np.zeros(cap, dtype=np.int64)
    qh, ql = np.zeros(cap, dtype=np.uint64), np.zeros(cap, dtype=np.uint64)
    res = CommunityResult()
    _check(call(labels.ctypes.data, level_labels.ctypes.data, cap, degree.ctypes.data, strength.ctypes.data, internal.ctypes.data,
                total.ctypes.data, MEM_HOST, lc.ctypes.data, lr.ctypes.data, qh.ctypes.data, ql.ctypes.data, ctypes.byref(res)))
    lv, cc = int(res.levels), int(res.communities)
    return Communities(res, labels, level_labels[:lv].copy(), degree, strength, internal[:cc].copy(), total[:cc].copy(),
                       lc[:lv].tolist(), lr[:lv].tolist(), [_i128(qh[i], ql[i]) for i in range(lv)])


def community_modularity(n, lo, hi, a, labels, resolution=1.0, g_fixed=None):
    """mvs_community_modularity (pure host): Qnum of `labels` on the graph of the raw edges (lo, hi, a: int64 weights,
    1 <= a < 2^55) at g = rint(resolution * 2^12), or at g_fixed -> Python int"""
    lo, hi = np.ascontiguousarray(lo, dtype=np.int32), np.ascontiguousarray(hi, dtype=np.int32)
    a, labels = np.ascontiguousarray(a, dtype=np.int64), np.ascontiguousarray(labels, dtype=np.int32)
    if not (len(lo) == len(hi) == len(a)) or len(labels) != n:
        raise ValueError("lo, hi and a must have one length, labels n entries")
    g = int(np.rint(resolution * COMMUNITY_R)) if g_fixed is None else int(g_fixed)
    qh, ql = _c.c_uint64(), _c.c_uint64()
    _check(load_library().mvs_community_modularity(int(n), lo.ctypes.data, hi.ctypes.data, a.ctypes.data, len(lo), labels.ctypes.data, g,
                                                   ctypes.byref(qh), ctypes.byref(ql)))
    return _i128(qh.value, ql.value)


TSNE_INIT = {"pcoa": 0, "random": 1}


class TsneGraph(_Handle):
    """The symmetric graph of integer affinities of n samples and the optimiser's state (y, velocity, gain) on the device
    (mvs_tsne_graph; include/mvs_hip.h "t-SNE"): feed it with add_neighbours (a top-k cell list, calibrated on the device) or
    add_edges (raw integer edges), finish_graph, then set_state / gradient / run / kl."""
    _destroy = "mvs_tsne_destroy"

    def __init__(self, ctx, n, _handle=None):
        self.ctx, self.n = ctx, int(n)
        if _handle is None:
            _handle = _P()
            _check(ctx.lib.mvs_tsne_create(ctx._h, self.n, ctypes.byref(_handle)))
        self._h = _handle
        ctx._children.add(self)

    def add_edges(self, lo, hi, s):
        """raw edges: three int32 arrays of one length (numpy, or torch tensors that all live in the same place), s >= 1"""
        if _is_torch(lo):
            (lp, lm, lk), (hp, hm, hk), (sp, sm, sk) = _buf(lo), _buf(hi), _buf(s)
            if not (lm == hm == sm):
                raise ValueError("lo, hi and s must live in the same place")
        else:
            (lp, lm, lk), (hp, hm, hk), (sp, sm, sk) = _buf(lo, np.int32), _buf(hi, np.int32), _buf(s, np.int32)
        if not (len(lo) == len(hi) == len(s)):
            raise ValueError("lo, hi and s must have one length")
        _check(self.ctx.lib.mvs_tsne_add_edges(self._h, lp, hp, sp, len(lo), lm))

    def add_neighbours(self, cells, norms_sq, d, perplexity, n_cells=None):
        """cells: a CELL_DTYPE array (host) or a torch CUDA int32 tensor [m, 4], sorted by row as pairwise_topk returns them
        -> (beta float64 [n]: written between the list's first and last row, c int32 per cell)"""
        if _is_torch(cells):
            cp, n_cells, ck = _cell_list(cells, n_cells)
            cm = MEM_DEVICE
        else:
            ck = np.ascontiguousarray(cells, dtype=CELL_DTYPE)
            cp, cm, n_cells = ck.ctypes.data, MEM_HOST, len(ck)
        np_, nm, nk = _norms(norms_sq)
        beta = np.zeros(self.n, dtype=np.float64)
        c = np.zeros(max(1, n_cells), dtype=np.int32)
        _check(self.ctx.lib.mvs_tsne_add_neighbours(self._h, cp, n_cells, cm, np_, nm, int(d), float(perplexity), beta.ctypes.data,
                                                    c.ctypes.data))
        return beta, c[:n_cells]

    def finish_graph(self):
        _check(self.ctx.lib.mvs_tsne_finish_graph(self._h))

    def edges(self):
        """-> (row, col, s, S): the stored directed entries sorted by (row, col) as int32 / int32 / int64 arrays, and their sum"""
        m, S = _c.c_int64(), _c.c_uint64()
        _check(self.ctx.lib.mvs_tsne_edges(self._h, None, None, None, 0, ctypes.byref(m), ctypes.byref(S)))
        row, col = np.zeros(max(1, m.value), dtype=np.int32), np.zeros(max(1, m.value), dtype=np.int32)
        s = np.zeros(max(1, m.value), dtype=np.int64)
        _check(self.ctx.lib.mvs_tsne_edges(self._h, row.ctypes.data, col.ctypes.data, s.ctypes.data, len(s), ctypes.byref(m), ctypes.byref(S)))
        return row[:m.value], col[:m.value], s[:m.value], int(S.value)

    def set_state(self, y=None, velocity=None, gain=None):
        """float64 [n, 2] each; None leaves that part as it is"""
        bufs = []
        for a in (y, velocity, gain):
            if a is None:
                bufs.append(None)
                continue
            a = np.ascontiguousarray(a, dtype=np.float64)
            if a.shape != (self.n, 2):
                raise ValueError("state arrays are [n, 2]")
            bufs.append(a)
        _check(self.ctx.lib.mvs_tsne_set_state(self._h, *[None if a is None else a.ctypes.data for a in bufs]))

    def get_state(self):
        """-> (y, velocity, gain), float64 [n, 2] each"""
        out = [np.zeros((self.n, 2), dtype=np.float64) for _ in range(3)]
        _check(self.ctx.lib.mvs_tsne_get_state(self._h, *[a.ctypes.data for a in out]))
        return tuple(out)

    def gradient(self, exaggeration=1.0):
        """one evaluation, state untouched -> (grad float64 [n, 2], Z_rows int64 [n], Z int)"""
        grad, zr, z = np.zeros((self.n, 2), dtype=np.float64), np.zeros(self.n, dtype=np.int64), _c.c_int64()
        _check(self.ctx.lib.mvs_tsne_gradient(self._h, float(exaggeration), grad.ctypes.data, zr.ctypes.data, ctypes.byref(z)))
        return grad, zr, int(z.value)

    def run(self, iterations, exaggeration, momentum, learning_rate):
        _check(self.ctx.lib.mvs_tsne_run(self._h, int(iterations), float(exaggeration), float(momentum), float(learning_rate)))

    def kl(self):
        v = _c.c_double()
        _check(self.ctx.lib.mvs_tsne_kl(self._h, ctypes.byref(v)))
        return v.value


class Tsne:
    """What Context.tsne returns: `coordinates` (float64 [n, 2], centred), `initial` (the state the optimiser started from),
    `beta` (float64 [n]; 0 = a uniform row), `kl`, `edges` (row, col, s, S of the symmetric graph), `iterations`,
    `learning_rate`, `neighbours`, `beta_zero_rows`."""

    def __init__(self, res, coordinates, initial, beta, edges):
        self.coordinates, self.initial, self.beta, self.edges = coordinates, initial, beta, edges
        self.kl, self.iterations, self.learning_rate = float(res.kl), int(res.iterations), float(res.learning_rate)
        self.neighbours, self.beta_zero_rows = int(res.neighbours), int(res.beta_zero_rows)

    def __repr__(self):
        return "Tsne(%d samples, %d neighbours, %d entries, %d iterations, KL %.4f)" % (
            len(self.coordinates), self.neighbours, len(self.edges[0]), self.iterations, self.kl)


class DerepResult:
    """What Derep.finish / Context.dereplicate return: numpy int32 arrays over the samples -- `rep_of` (the sample's
    representative, itself for a representative), `link_dot` / `link_q` (dot and q of the cell (i, rep_of[i]); 0 and -1 for a
    representative), `sizes` (samples assigned to i, itself included; 0 for a member) -- and `is_rep`, `representatives` (the
    ascending indices), `n_representatives`."""

    def __init__(self, rep_of, link_dot, link_q, sizes):
        self.rep_of, self.link_dot, self.link_q, self.sizes = rep_of, link_dot, link_q, sizes
        self.is_rep = rep_of == np.arange(len(rep_of), dtype=np.int32)
        self.representatives = np.flatnonzero(self.is_rep).astype(np.int32)
        self.n_representatives = len(self.representatives)

    def jaccard(self, norms_sq, d):
        """the fp64 Jaccard estimate of every sample to its representative, in mvs_pairwise_topk's order of operations
        (inter = dot / d; J = inter / (n2[i] + n2[rep] - inter)); 1.0 for a representative"""
        n2 = np.asarray(norms_sq, dtype=np.float64)
        inter = self.link_dot.astype(np.float64) / float(d)
        with np.errstate(all="ignore"):
            j = inter / (n2 + n2[self.rep_of] - inter)
        j[self.is_rep] = 1.0
        return j

    def __repr__(self):
        return "DerepResult(%d samples, %d representatives, largest %d)" % (
            len(self.rep_of), self.n_representatives, int(self.sizes.max()) if len(self.sizes) else 0)


class Derep(_Handle):
    """Greedy dereplication of n samples in ROW order (mvs_derep): row 0 goes first, a row becomes a representative iff no
    representative before it is linked to it.  Feed it row block by row block with add_rows (each list holds every cell
    (r, c), c < r, of the block's rows) or in one go with Context.derep_into, read it with finish."""
    _destroy = "mvs_derep_destroy"

    def __init__(self, ctx, n):
        self.ctx, self.n = ctx, int(n)
        h = _P()
        _check(ctx.lib.mvs_derep_create(ctx._h, self.n, ctypes.byref(h)))
        self._h = h
        ctx._children.add(self)

    def add_rows(self, cells, row_begin, row_end, n_cells=None):
        """cells: torch CUDA tensor (int32 [m, 4]; the first n_cells rows, default all) or a device address (int) with n_cells:
        the cells of rows [row_begin, row_end); row_begin must continue the rows decided so far"""
        cp, n_cells, ck = _cell_list(cells, n_cells)
        _check(self.ctx.lib.mvs_derep_add_rows(self._h, cp, n_cells, int(row_begin), int(row_end)))

    def finish(self, order=None):
        """-> DerepResult in the caller's index space: order (int32 permutation, numpy or torch; None = identity) says which
        sample each row is"""
        op, om = None, MEM_HOST
        if order is not None:
            op, om, ok = _buf(order) if _is_torch(order) else _buf(order, np.int32)
            if len(order) != self.n:
                raise ValueError("order must have n entries")
        n = self.n
        rep_of, link_dot = np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int32)
        link_q, sizes = np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int32)
        count = _c.c_int64()
        _check(self.ctx.lib.mvs_derep_finish(self._h, op, om, rep_of.ctypes.data, link_dot.ctypes.data, link_q.ctypes.data,
                                             sizes.ctypes.data, MEM_HOST, ctypes.byref(count)))
        res = DerepResult(rep_of, link_dot, link_q, sizes)
        assert res.n_representatives == count.value
        return res


class LinkageResult:
    """What Linkage.finish / Context.linkage return: the maximum spanning forest of the thresholded Jaccard graph -- the
    single-linkage tree -- as numpy arrays `a`, `b` (the link's samples, a < b), `dot`, `q` (int32) and `jaccard` (float64),
    sorted best first (jaccard descending, then a, then b), and `n`, the number of samples."""

    def __init__(self, n, links):
        self.n = int(n)
        self.a, self.b = np.ascontiguousarray(links["a"]), np.ascontiguousarray(links["b"])
        self.dot, self.q = np.ascontiguousarray(links["dot"]), np.ascontiguousarray(links["q"])
        self.jaccard = np.ascontiguousarray(links["jaccard"])

    def __len__(self):
        return len(self.a)

    def _merge(self, count):
        """union-find over the first `count` links -> (root of every sample, size of the merged cluster after each link)"""
        parent = list(range(self.n))
        size = [1] * self.n
        merged = np.empty(count, dtype=np.int64)

        def find(x):
            while parent[x] != x:
                parent[x] = parent[parent[x]]
                x = parent[x]
            return x
        for i, (a, b) in enumerate(zip(self.a[:count].tolist(), self.b[:count].tolist())):
            ra, rb = find(a), find(b)
            if ra != rb:                              # (always: a forest has no cycle)
                lo, hi = min(ra, rb), max(ra, rb)
                parent[hi] = lo
                size[lo] += size[hi]
                ra = lo
            merged[i] = size[ra]
        return np.array([find(i) for i in range(self.n)], dtype=np.int64), merged

    def cut(self, level):
        """-> (labels, sizes) of the clusters at Jaccard > level (level >= the level the forest was built at): the components
        of the links with jaccard > level, a prefix of the list; clusters numbered by ascending smallest member, as
        ClusterResult numbers them"""
        with np.errstate(invalid="ignore"):
            above = self.jaccard > level
        count = int(above.sum())
        assert not above[count:].any()
        roots, _ = self._merge(count)
        uniq = np.unique(roots)                       # a root is its cluster's smallest member
        labels = np.searchsorted(uniq, roots).astype(np.int32)
        return labels, np.bincount(labels, minlength=len(uniq)).astype(np.int32)

    def merge_sizes(self):
        """the size of the merged cluster after each link, in the list's order (int64)"""
        return self._merge(len(self))[1]

    def __repr__(self):
        return "LinkageResult(%d samples, %d links)" % (self.n, len(self))


class Linkage(_Handle):
    """The single-linkage tree of n samples, built on the device from lists of cells (mvs_linkage): the maximum spanning
    forest of everything it was fed, under the order (jaccard descending, a, b).  norms_sq (n doubles) and d decide every
    weight.  Feed it with add_cells (any device list with real dots: the output of Context.search_block / pairwise_block, a
    torch int32 tensor [m, 4] or a raw device pointer) or Context.linkage_into; read it with finish or cells."""
    _destroy = "mvs_linkage_destroy"

    def __init__(self, ctx, n, d, norms_sq):
        self.ctx, self.n, self.d = ctx, int(n), int(d)
        np_, nm, nk = _norms(norms_sq)
        if len(norms_sq) != self.n:
            raise ValueError("norms_sq must hold n values")
        h = _P()
        _check(ctx.lib.mvs_linkage_create(ctx._h, self.n, self.d, np_, nm, ctypes.byref(h)))
        self._h = h
        ctx._children.add(self)

    def set_core(self, core):
        """mvs_linkage_set_core: from now on the weight of a link is the mutual reachability min(jaccard, core[a], core[b]) --
        the `jaccard` of every result then holds that value.  core: n doubles (numpy or torch, host or device), e.g. what
        Context.core_jaccard returns.  Only before the first cell is fed."""
        cp, cm, ck = _norms(core)
        if len(core) != self.n:
            raise ValueError("core must hold n values")
        _check(self.ctx.lib.mvs_linkage_set_core(self._h, cp, cm))

    def add_cells(self, cells, n_cells=None):
        """cells: torch CUDA tensor (int32 [m, 4]; the first n_cells rows, default all) or a device address (int) with n_cells.
        Feeding a list twice changes nothing."""
        cp, n_cells, ck = _cell_list(cells, n_cells)
        _check(self.ctx.lib.mvs_linkage_add_cells(self._h, cp, n_cells))

    def finish(self, capacity=None):
        """-> LinkageResult.  capacity: room for that many links (default n - 1, which always suffices); too little raises
        MvsError MVS_E_CAPACITY with `needed`."""
        if capacity is None:
            capacity = max(self.n - 1, 0)
        links = np.empty(max(int(capacity), 1), dtype=LINK_DTYPE)
        count = _c.c_int64()
        rc = self.ctx.lib.mvs_linkage_finish(self._h, links.ctypes.data, int(capacity), MEM_HOST, ctypes.byref(count))
        if rc == MVS_E_CAPACITY:
            raise MvsError(rc, self.ctx.lib.mvs_last_error().decode("utf-8", "replace"), needed=count.value)
        _check(rc)
        return LinkageResult(self.n, links[:count.value])

    def cells(self, level, out=None):
        """the links with jaccard > level as a device cell list, best first -> (torch int32 tensor [capacity, 4], count):
        ready for Cluster.add_cells and Context.intersect_cells.  out: a device tensor to write into (default: room for
        n - 1 cells); too little room raises MvsError MVS_E_CAPACITY with `needed`."""
        if out is None:
            import torch
            out = torch.empty((max(self.n - 1, 1), 4), dtype=torch.int32, device=torch.device("cuda", self.ctx.device))
        op, om, ok = _buf(out)
        if om != MEM_DEVICE:
            raise ValueError("out must be a device buffer")
        count = _c.c_int64()
        rc = self.ctx.lib.mvs_linkage_cells(self._h, float(level), op, out.shape[0], ctypes.byref(count))
        if rc == MVS_E_CAPACITY:
            raise MvsError(rc, self.ctx.lib.mvs_last_error().decode("utf-8", "replace"), needed=count.value)
        _check(rc)
        return out, count.value


class Hdbscan:
    """What hdbscan_select / Context.hdbscan return (include/mvs_hip.h "HDBSCAN*"): `labels` int32 [n] (the rank of the sample's
    selected cluster, -1 noise), `strength` float64 [n], `lambda_out` int64 [n] (the level at which the sample left its last
    cluster, -1 never in one), `clusters` (HDBSCAN_CLUSTER_DTYPE: parent, size, selected, representative, birth, death,
    stability -- every condensed cluster, by smallest member then size descending); from Context.hdbscan also `core` float64
    [n] and `links` (a LinkageResult whose `jaccard` is the mutual reachability).  Levels are llrint(clamp(x, 0, 1) * 2^30)."""

    def __init__(self, labels, strength, lambda_out, clusters, core=None, links=None):
        self.labels, self.strength, self.lambda_out, self.clusters, self.core, self.links = labels, strength, lambda_out, clusters, core, links
        self.n_clusters = int(clusters["selected"].sum())

    def __repr__(self):
        return "Hdbscan(%d samples, %d clusters of %d condensed, %d noise)" % (len(self.labels), self.n_clusters, len(self.clusters),
                                                                               int((self.labels < 0).sum()))


def _links_array(links):
    """a LinkageResult, a dict of arrays or a LINK_DTYPE array -> LINK_DTYPE array"""
    if isinstance(links, np.ndarray) and links.dtype == LINK_DTYPE:
        return np.ascontiguousarray(links)
    get = (lambda f: links[f]) if isinstance(links, dict) else (lambda f: getattr(links, f))
    out = np.zeros(len(get("a")), dtype=LINK_DTYPE)
    for f in LINK_DTYPE.names:
        out[f] = get(f)
    return out


def hdbscan_select(n, links, core=None, floor=0.05, min_cluster_size=5, allow_roots=True):
    """mvs_hdbscan_select: condensed tree and selection by excess of mass over the links of a linkage built under the mutual
    reachability (Linkage.set_core), best first -> Hdbscan.  links: a LinkageResult, a dict of arrays a / b / dot / q / jaccard or
    a LINK_DTYPE array; core: n doubles or None (decides the representatives only).  Needs no device."""
    arr = _links_array(links)
    n = int(n)
    labels, strength = np.full(n, -1, dtype=np.int32), np.zeros(n, dtype=np.float64)
    lam = np.full(n, -1, dtype=np.int64)
    clusters = np.zeros(max(n, 1), dtype=HDBSCAN_CLUSTER_DTYPE)
    core_a = None if core is None else np.ascontiguousarray(core, dtype=np.float64)
    if core_a is not None and len(core_a) != n:
        raise ValueError("core must hold n values")
    count = _c.c_int64()
    _check(load_library().mvs_hdbscan_select(n, arr.ctypes.data, len(arr), None if core_a is None else core_a.ctypes.data, float(floor),
                                             int(min_cluster_size), 0 if allow_roots else HDBSCAN_NO_ROOTS, labels.ctypes.data,
                                             strength.ctypes.data, lam.ctypes.data, clusters.ctypes.data, len(clusters), ctypes.byref(count)))
    return Hdbscan(labels, strength, lam, clusters[:count.value].copy(), core_a)


class Pca(_Handle):
    """A fitted PCA of the rows of a sketch set (mvs_pca; Context.pca makes one): numpy float64 arrays `mean` [d], `axes` [c, d]
    (unit length, one axis per row), `explained_variance` [c] (the eigenvalues of the covariance, descending),
    `explained_variance_ratio` [c] (explained_variance / total_variance), `residuals` [c] (||C v - lambda v||_2 of every
    returned pair); `iterations`, `converged`, `n` (fitted samples), `total_variance`.  Closes with its context."""
    _destroy = "mvs_pca_destroy"

    def __init__(self, ctx, handle):
        self.ctx, self._h = ctx, handle
        ctx._children.add(self)
        d, c, n, it, cv, tv = _c.c_int(), _c.c_int(), _c.c_int64(), _c.c_int(), _c.c_int(), _c.c_double()
        _check(ctx.lib.mvs_pca_info(handle, ctypes.byref(d), ctypes.byref(c), ctypes.byref(n), ctypes.byref(it), ctypes.byref(cv),
                                    ctypes.byref(tv)))
        self.d, self.components, self.n = d.value, c.value, n.value
        self.iterations, self.converged, self.total_variance = it.value, bool(cv.value), tv.value
        self.mean = np.empty(self.d, dtype=np.float64)
        self.axes = np.empty((self.components, self.d), dtype=np.float64)
        self.explained_variance = np.empty(self.components, dtype=np.float64)
        self.residuals = np.empty(self.components, dtype=np.float64)
        _check(ctx.lib.mvs_pca_get(handle, self.mean.ctypes.data, self.axes.ctypes.data, self.explained_variance.ctypes.data,
                                   self.residuals.ctypes.data))
        with np.errstate(all="ignore"):
            self.explained_variance_ratio = self.explained_variance / self.total_variance

    def transform(self, sset, row_begin=0, row_end=None):
        """scores of rows [row_begin, row_end) of `sset` -- the fitted set or any other of the same dimension -- on the axes:
        float64 [rows, c], sum_a (x[i][a] - mean[a]) * axes[j][a]"""
        if self._h is None:
            raise ValueError("the pca is closed")
        if row_end is None:
            row_end = sset.n
        rows = max(0, int(row_end) - int(row_begin))
        out = np.empty((rows, self.components), dtype=np.float64)
        _check(self.ctx.lib.mvs_pca_transform(self.ctx._h, self._h, sset._h, int(row_begin), int(row_end), out.ctypes.data, MEM_HOST))
        return out


class Permanova:
    """The result of Context.permanova (mvs_permanova): f, p_value, r2, ss_total, ss_within, ss_between, df_between, df_within,
    samples, groups (the non-empty ones), permutations; group_sizes int64 and group_mean_d2 float64 per group id (the mean
    squared distance inside the group, 0 for a singleton); perm_f float64 [permutations], the pseudo-F of every relabelling"""

    def __init__(self, res, group_sizes, group_mean_d2, perm_f):
        for name, _ in PermanovaResult._fields_:
            setattr(self, name, getattr(res, name))
        self.group_sizes, self.group_mean_d2, self.perm_f = group_sizes, group_mean_d2, perm_f


def permutation_labels(labels, permutations, seed=0):
    """mvs_permutation_labels: labels uint8 [m] -> uint8 [permutations + 1, m]; row 0 is `labels`, row p a shuffle of it that is
    a function of (seed, p) alone.  Needs no device."""
    lab = np.ascontiguousarray(labels, dtype=np.uint8)
    if lab.ndim != 1:
        raise ValueError("labels must be one-dimensional")
    out = np.zeros((max(0, int(permutations)) + 1, len(lab)), dtype=np.uint8)
    _check(load_library().mvs_permutation_labels(lab.ctypes.data, len(lab), int(permutations), int(seed) & (2 ** 64 - 1), out.ctypes.data))
    return out


def permanova_stats(sums, sizes, m):
    """mvs_permanova_stats: sums [permutations + 2, groups] of Python ints and sizes int64 of the same shape, the last slot the
    all-zero labelling -> Permanova (group_sizes: those of slot 0).  Needs no device."""
    sizes = np.ascontiguousarray(sizes, dtype=np.int64)
    slots, groups = sizes.shape
    flat = [int(v) for v in np.asarray(sums, dtype=object).reshape(-1)]
    lo = np.array([v & (2 ** 64 - 1) for v in flat], dtype=np.uint64)
    hi = np.array([v >> 64 for v in flat], dtype=np.uint64)
    res = PermanovaResult()
    mean = np.zeros(groups, dtype=np.float64)
    perm_f = np.zeros(max(0, slots - 2), dtype=np.float64)
    _check(load_library().mvs_permanova_stats(lo.ctypes.data, hi.ctypes.data, sizes.ctypes.data, slots - 2, groups, int(m), ctypes.byref(res),
                                              mean.ctypes.data, perm_f.ctypes.data))
    return Permanova(res, sizes[0].copy(), mean, perm_f)


class Silhouette:
    """The result of Context.silhouette (mvs_silhouette) or silhouette_stats: per sample of the range `samples` (the silhouette s),
    `a`, `b`, `centroid_d2` float64 and `nearest` int32 (s, a and centroid_d2 are NaN for an unlabelled sample); `mean` (of s over
    the labelled samples), `negative` (labelled samples with s < 0), `labelled`, `groups` (the non-empty ones); per group id
    `group_sizes` int64, `group_mean` (of s), `group_within` (mean distance inside the group), `group_dispersion` (mean
    centroid_d2) float64 and `medoids` int64 (an index into the range, -1 for an empty group)"""

    def __init__(self, res, samples, a, b, nearest, centroid_d2, group_sizes, group_mean, group_within, group_dispersion, medoids):
        self.mean, self.negative, self.labelled, self.groups = res.mean, res.negative, res.labelled, res.groups
        self.samples, self.a, self.b, self.nearest, self.centroid_d2 = samples, a, b, nearest, centroid_d2
        self.group_sizes, self.group_mean, self.group_within, self.group_dispersion, self.medoids = \
            group_sizes, group_mean, group_within, group_dispersion, medoids


def _labels(labels, m=None):
    lab = np.ascontiguousarray(labels, dtype=np.int32)
    if lab.ndim != 1 or (m is not None and len(lab) != m):
        raise ValueError("labels must have one entry per row of the range")
    return lab


def silhouette_stats(labels, sizes, own_sum, near_group, near_sum):
    """mvs_silhouette_stats: labels int32 [m] (-1: unlabelled), sizes int64 [groups] and the three arrays of Context.label_sums
    -> Silhouette.  Needs no device."""
    lab = _labels(labels)
    m = len(lab)
    sizes = np.ascontiguousarray(sizes, dtype=np.int64)
    groups = len(sizes)
    own = np.ascontiguousarray(own_sum, dtype=np.uint64)
    near = np.ascontiguousarray(near_group, dtype=np.int32)
    nsum = np.ascontiguousarray(near_sum, dtype=np.uint64)
    if not (len(own) == len(near) == len(nsum) == m):
        raise ValueError("the arrays must have one entry per label")
    res = SilhouetteResult()
    s, a, b, c2 = (np.zeros(m, dtype=np.float64) for _ in range(4))
    gm, gw, gd = (np.zeros(groups, dtype=np.float64) for _ in range(3))
    med = np.zeros(groups, dtype=np.int64)
    _check(load_library().mvs_silhouette_stats(lab.ctypes.data, m, groups, sizes.ctypes.data, own.ctypes.data, near.ctypes.data, nsum.ctypes.data,
                                               ctypes.byref(res), s.ctypes.data, a.ctypes.data, b.ctypes.data, c2.ctypes.data, gm.ctypes.data,
                                               gw.ctypes.data, gd.ctypes.data, med.ctypes.data))
    return Silhouette(res, s, a, b, near.copy(), c2, sizes.copy(), gm, gw, gd, med)


def _hclust_method(method):
    """'average' / 'complete' (or the ABI's number) -> MVS_HCLUST_*"""
    if isinstance(method, str):
        if method not in HCLUST_METHODS:
            raise ValueError("method must be one of %s" % sorted(HCLUST_METHODS))
        return HCLUST_METHODS[method]
    return int(method)


def _merges(m, merges):
    mg = np.ascontiguousarray(merges, dtype=HMERGE_DTYPE)
    if mg.ndim != 1 or len(mg) != max(0, int(m) - 1):
        raise ValueError("a tree of m leaves has m - 1 merges")
    return mg


def hclust_order(m, merges):
    """mvs_hclust_order: the m - 1 records of a Hclust -> SciPy's linkage matrix, float64 [m - 1, 4]: the merges sorted by
    (height, round, a), a leaf's id its index, the t-th merge's id m + t.  Needs no device."""
    mg = _merges(m, merges)
    Z = np.zeros((len(mg), 4), dtype=np.float64)
    _check(load_library().mvs_hclust_order(int(m), mg.ctypes.data, Z.ctypes.data))
    return Z


def hclust_cut(m, merges, height=None, clusters=None):
    """mvs_hclust_cut (height: the merges with height <= it) or mvs_hclust_cut_count (clusters: the first m - clusters merges
    of the sorted order) -> labels int32 [m], 0-based in ascending order of each cluster's smallest member.  Needs no device."""
    if (height is None) == (clusters is None):
        raise ValueError("give either height or clusters")
    mg = _merges(m, merges)
    labels = np.zeros(int(m), dtype=np.int32)
    if height is not None:
        _check(load_library().mvs_hclust_cut(int(m), mg.ctypes.data, float(height), labels.ctypes.data))
    else:
        _check(load_library().mvs_hclust_cut_count(int(m), mg.ctypes.data, int(clusters), labels.ctypes.data))
    return labels


class Hclust:
    """The result of Context.hclust / hclust_weights / hclust_sums: `merges`, the m - 1 records (HMERGE_DTYPE: a < b the slots,
    round, size, sum, height) in (round, a) order; `rounds`; `m`; `method` (0 average, 1 complete)"""

    def __init__(self, m, method, merges, rounds):
        self.m, self.method, self.merges, self.rounds = int(m), int(method), merges, int(rounds)

    def linkage_matrix(self):
        """-> SciPy's linkage matrix (hclust_order)"""
        return hclust_order(self.m, self.merges)

    def cut(self, height):
        """-> labels int32 [m] after the merges with height <= `height`"""
        return hclust_cut(self.m, self.merges, height=height)

    def cut_count(self, k):
        """-> labels int32 [m] of k clusters"""
        return hclust_cut(self.m, self.merges, clusters=k)


class Pcoa(_Handle):
    """Principal coordinates of the Jaccard estimates of the rows [row_begin, row_end) of a sketch set (mvs_pcoa; Context.pcoa
    makes one): numpy float64 arrays `eigenvalues` [c] (of B = 1/2 H K H, descending), `vectors` [m, c] (unit columns),
    `coordinates` [m, c] (sqrt(max(eigenvalue, 0)) * vector), `row_means` [m], `explained_ratio` [c] (eigenvalues / trace),
    `residuals` [c] (||B v - lambda v||_2 of every returned pair); `grand_mean`, `trace`, `iterations`, `converged`,
    `negative_ritz` (negative Ritz values in the solver's final block), `floor`.  The iteration finds the eigenvalues of
    largest magnitude: see include/mvs_hip.h.  Closes with its context."""
    _destroy = "mvs_pcoa_destroy"

    def __init__(self, ctx, handle, sset, norms_sq):
        self.ctx, self._h, self.sset, self.norms_sq = ctx, handle, sset, norms_sq
        ctx._children.add(self)
        rb, re = _c.c_int64(), _c.c_int64()
        c, blk, it, cv, neg = _c.c_int(), _c.c_int(), _c.c_int(), _c.c_int(), _c.c_int()
        fl, gm, tr = _c.c_double(), _c.c_double(), _c.c_double()
        _check(ctx.lib.mvs_pcoa_info(handle, ctypes.byref(rb), ctypes.byref(re), ctypes.byref(c), ctypes.byref(blk), ctypes.byref(it),
                                     ctypes.byref(cv), ctypes.byref(neg), ctypes.byref(fl), ctypes.byref(gm), ctypes.byref(tr)))
        self.row_begin, self.row_end, self.components, self.block = rb.value, re.value, c.value, blk.value
        self.n = self.row_end - self.row_begin
        self.iterations, self.converged, self.negative_ritz = it.value, bool(cv.value), neg.value
        self.floor, self.grand_mean, self.trace = fl.value, gm.value, tr.value
        self.eigenvalues = np.empty(self.components, dtype=np.float64)
        self.vectors = np.empty((self.n, self.components), dtype=np.float64)
        self.coordinates = np.empty((self.n, self.components), dtype=np.float64)
        self.row_means = np.empty(self.n, dtype=np.float64)
        self.residuals = np.empty(self.components, dtype=np.float64)
        _check(ctx.lib.mvs_pcoa_get(handle, self.eigenvalues.ctypes.data, self.vectors.ctypes.data, self.coordinates.ctypes.data,
                                    self.row_means.ctypes.data, self.residuals.ctypes.data))
        with np.errstate(all="ignore"):
            self.explained_ratio = self.eigenvalues / self.trace

    def transform(self, rows=None, norms_sq=None):
        """Gower's out-of-sample scores of `rows` = (begin, end) of the fitted set handle (default: every row of it, the
        samples appended behind the fitted ones included): float64 [rows, c].  norms_sq: the set's squared norms (default:
        those the fit was given)."""
        if self._h is None:
            raise ValueError("the pcoa is closed")
        rb, re = (0, self.sset.n) if rows is None else rows
        np_, nm, nk = _norms(self.norms_sq if norms_sq is None else norms_sq)
        out = np.empty((max(0, int(re) - int(rb)), self.components), dtype=np.float64)
        _check(self.ctx.lib.mvs_pcoa_transform(self.ctx._h, self._h, self.sset._h, np_, nm, int(rb), int(re), out.ctypes.data, MEM_HOST))
        return out


class HashSet(_Handle):
    """Hash lists of n samples resident in HBM, per sample sorted and de-duplicated (mvs_hash_set): what
    Context.intersect_cells intersects.  `n` samples, `total` distinct hashes, `was_sorted`: the input was already strictly
    increasing inside every sample (it is then used as uploaded)."""
    _destroy = "mvs_hash_set_destroy"

    def __init__(self, ctx, handle):
        self.ctx, self._h = ctx, handle
        ctx._children.add(self)
        n, total, ws = _c.c_int64(), _c.c_int64(), _c.c_int()
        _check(ctx.lib.mvs_hash_set_info(handle, ctypes.byref(n), ctypes.byref(total), ctypes.byref(ws)))
        self.n, self.total, self.was_sorted = n.value, total.value, bool(ws.value)

    def sizes(self, out=None):
        """distinct hashes per sample: numpy int32 [n], or written into `out` (numpy or a torch device tensor)"""
        if out is None:
            out = np.empty(self.n, dtype=np.int32)
        op, om, ok = _buf(out, np.int32, writable=True) if not _is_torch(out) else _buf(out)
        _check(self.ctx.lib.mvs_hash_set_sizes(self._h, op, om))
        return out

    def export(self):
        """-> (hashes uint64 [total], offsets int64 [n + 1]) as numpy arrays: every sample's values, strictly increasing
        (mvs_hash_set_export)"""
        hashes, offsets = np.empty(self.total, dtype=np.uint64), np.empty(self.n + 1, dtype=np.int64)
        _check(self.ctx.lib.mvs_hash_set_export(self._h, hashes.ctypes.data, MEM_HOST, offsets.ctypes.data))
        return hashes, offsets

    def device_hashes(self):
        """-> DeviceArray of the set's values where they lie (mvs_hash_set_device), valid while the set is open: with
        export()'s offsets (or offsets()), Context.project_csr projects the set without a copy over the link"""
        if self._h is None:
            raise ValueError("the hash set is closed")
        p = _P()
        _check(self.ctx.lib.mvs_hash_set_device(self._h, ctypes.byref(p)))
        return DeviceArray(p.value, self.total, np.uint64, self)

    def offsets(self):
        """-> int64 [n + 1]: where every sample's values start in export()'s / device_hashes()'s array"""
        offsets = np.empty(self.n + 1, dtype=np.int64)
        _check(self.ctx.lib.mvs_hash_set_export(self._h, None, MEM_HOST, offsets.ctypes.data))
        return offsets

    def abundances(self):
        """-> uint32 [total]: the abundance of every value, aligned with export()'s values (mvs_hash_set_abundances), or None
        for a set that carries none: only KmerSketcher.finish and Context.hash_set_counted make sets that do"""
        if self._h is None:
            raise ValueError("the hash set is closed")
        out = np.empty(self.total, dtype=np.uint32)
        rc = self.ctx.lib.mvs_hash_set_abundances(self._h, out.ctypes.data, MEM_HOST)
        if rc == MVS_E_INVALID:
            return None
        _check(rc)
        return out

    def abundance_totals(self):
        """-> (sum, sumsq_lo, sumsq_hi), uint64 [n] each: per sample the sum S of the abundances and the sum Q of their squares
        as Q = sumsq_hi * 2^32 + sumsq_lo (mvs_hash_set_abundance_totals).  A set that carries no abundances counts 1 per
        value: S = sumsq_lo = the sample's size, sumsq_hi = 0."""
        if self._h is None:
            raise ValueError("the hash set is closed")
        out = [np.zeros(self.n, dtype=np.uint64) for _ in range(3)]
        _check(self.ctx.lib.mvs_hash_set_abundance_totals(self._h, out[0].ctypes.data, out[1].ctypes.data, out[2].ctypes.data, MEM_HOST))
        return tuple(out)


class KmerSketcher(_Handle):
    """The k-mer abundances of n read sets, fed over any number of calls (mvs_kmer_sketcher, include/mvs_hip.h "abundances").
    add() takes pieces -- byte strings no k-mer may span, each with its sample's index --, finish() returns the HashSet of the
    values whose abundance passes the filter; that set carries the abundances (HashSet.abundances) and outlives the sketcher."""
    _destroy = "mvs_kmer_sketcher_destroy"

    def __init__(self, ctx, n_samples, ksize=31, scaled=1000, seed=42, max_hash=None):
        if max_hash is None:
            max_hash = kmer_max_hash(scaled)
        h = _P()
        _check(ctx.lib.mvs_kmer_sketcher_create(ctx._h, int(n_samples), int(ksize), int(seed) & 0xFFFFFFFF, int(max_hash), ctypes.byref(h)))
        self.ctx, self._h, self.n = ctx, h, int(n_samples)
        self.histogram = None
        ctx._children.add(self)

    def _handle(self):
        if self._h is None:
            raise ValueError("the sketcher is closed")
        return self._h

    def add(self, pieces, samples):
        """pieces: a list of bytes / str, or a pair (bases, offsets) as Context.sketch_sequences takes it; samples: the sample
        index of every piece"""
        samples = np.ascontiguousarray(samples, dtype=np.int32)
        if isinstance(pieces, tuple) and len(pieces) == 2 and not isinstance(pieces[0], (bytes, bytearray, str)):
            bases, offsets = pieces
            offsets = np.ascontiguousarray(offsets, dtype=np.int64)
            if _is_torch(bases):
                if str(bases.dtype) != "torch.uint8":
                    raise ValueError("bases must be uint8")
                bp, bm, bk = _buf(bases)
            else:
                bp, bm, bk = _buf(bases, np.uint8)
        else:
            parts = [x.encode("latin-1") if isinstance(x, str) else bytes(x) for x in pieces]
            offsets = np.zeros(len(parts) + 1, dtype=np.int64)
            if parts:
                np.cumsum([len(x) for x in parts], out=offsets[1:])
            bp, bm, bk = _buf(np.frombuffer(b"".join(parts), dtype=np.uint8), np.uint8)
        if offsets.ndim != 1 or len(offsets) != len(samples) + 1:
            raise ValueError("offsets must hold one entry more than samples")
        _check(self.ctx.lib.mvs_kmer_sketcher_add(self._handle(), bp, bm, offsets.ctypes.data, samples.ctypes.data, len(samples)))

    def finish(self, min_abundance=1, max_abundance=0, histogram=False):
        """-> HashSet of the values v with min_abundance <= abundance(v) (<= max_abundance if that is > 0).  histogram=True also
        leaves int64 [n, 256] in self.histogram: distinct values per min(abundance, 255), before the filter"""
        hist = np.zeros((self.n, 256), dtype=np.int64) if histogram else None
        h = _P()
        _check(self.ctx.lib.mvs_kmer_sketcher_finish(self._handle(), int(min_abundance), int(max_abundance),
                                                      hist.ctypes.data if histogram else None, ctypes.byref(h)))
        self.histogram = hist
        return HashSet(self.ctx, h)

    def info(self):
        """-> dict of what this sketcher's calls did so far: kernel_ms (hashing passes and finish's scatter, timing on), staged
        pairs, capacity of the staging list (0 after finish), adds that hashed something, second_trips, growths of the list"""
        ms = _c.c_double()
        v = [_c.c_int64() for _ in range(5)]
        _check(self.ctx.lib.mvs_kmer_sketcher_info(self._handle(), ctypes.byref(ms), *[ctypes.byref(x) for x in v]))
        return dict(zip(("kernel_ms", "staged", "capacity", "adds", "second_trips", "growths"), [ms.value] + [x.value for x in v]))

    def stats(self):
        """-> dict of int64 [n] arrays: bases given, kmers (valid positions), kept (values <= max_hash, duplicates included), and
        after finish distinct values and those that passed the filter (zeros before)"""
        names = ("bases", "kmers", "kept", "distinct", "passed")
        out = {k: np.zeros(self.n, dtype=np.int64) for k in names}
        _check(self.ctx.lib.mvs_kmer_sketcher_stats(self._handle(), *[out[k].ctypes.data for k in names]))
        return out


class GatherResult:
    """What Context.gather returns: `matches` (GATHER_DTYPE records in the order the walk found them: sample, intersect =
    |Q n H|, unique = the hashes this match added, remaining = the query's hashes still unexplained after it), `query_size` =
    |Q|, `db_sizes` = |H| of every matched sample (int32, one per record).  SearchIndex.gather also sets `query_name` and
    `names` (the matched samples' names)."""

    def __init__(self, matches, query_size, db_sizes):
        self.matches, self.query_size, self.db_sizes = matches, int(query_size), db_sizes
        self.query_name, self.names = None, None

    def __len__(self):
        return len(self.matches)

    def fractions(self):
        """-> (f_orig_query, f_match, f_unique_to_query): intersect / |Q|, intersect / |H|, unique / |Q|, float64"""
        inter = self.matches["intersect"].astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            return (inter / float(self.query_size), inter / self.db_sizes.astype(np.float64),
                    self.matches["unique"].astype(np.float64) / float(self.query_size))

    @property
    def explained(self):
        """hashes of the query that the matches explain: the sum of `unique` = |Q| - the last `remaining`"""
        return int(self.matches["unique"].sum())


COMM_ID_BYTES = 128
PLAN_MIRROR_OUTSIDE = 1
CELLS_HEADER_BYTES = 64
WIRE_MAX_ABS = 32004          # mvs_sketch_set_planes_from_wire: largest |v| for which the low limb pins the value
PLAN_STALE = 1 << 62          # mvs_plan_finish under option plan_speculate: the cell count of a plan that must run again


class Comm(_Handle):
    """Communicator of the multi-GPU exchange step (mvs_comm): RCCL (one process per GPU), the file transport
    (ranks sharing a device), or caller-supplied collectives."""
    _destroy = "mvs_comm_destroy"

    def __init__(self, ctx, handle, keep=None):
        self.ctx, self._h, self._keep = ctx, handle, keep
        ctx._comms.add(self)             # a communicator holds a pointer to its context: closed before the context is
        r, w, k = _c.c_int(), _c.c_int(), _c.c_int()
        _check(ctx.lib.mvs_comm_info(handle, r, w, k))
        self.rank, self.world, self.is_rccl = r.value, w.value, bool(k.value)

    def allgather_planes(self, planes, rows_per_rank, limbs, d_pad):
        pp, pm, pk = _buf(planes)
        if pm != MEM_DEVICE:
            raise ValueError("planes must be a device buffer")
        _check(self.ctx.lib.mvs_allgather_planes(self.ctx._h, self._h, pp, int(rows_per_rank), int(limbs), int(d_pad)))

    def allgather_rows(self, planes, rows_per_rank, row_first, row_count, limbs, d_pad):
        pp, pm, pk = _buf(planes)
        if pm != MEM_DEVICE:
            raise ValueError("planes must be a device buffer")
        _check(self.ctx.lib.mvs_allgather_rows(self.ctx._h, self._h, pp, int(rows_per_rank), int(row_first), int(row_count),
                                               int(limbs), int(d_pad)))

    def allgather_f64(self, values, count_per_rank):
        vp, vm, vk = _buf(values)
        if vm != MEM_DEVICE:
            raise ValueError("values must be a device buffer")
        _check(self.ctx.lib.mvs_allgather_f64(self.ctx._h, self._h, vp, int(count_per_rank)))

    def allgather_bytes(self, buf, bytes_per_rank):
        bp, bm, bk = _buf(buf)
        if bm != MEM_DEVICE:
            raise ValueError("buf must be a device buffer")
        _check(self.ctx.lib.mvs_allgather_bytes(self.ctx._h, self._h, bp, int(bytes_per_rank)))

    def allreduce_max(self, value):
        v = _c.c_int64(int(value))
        _check(self.ctx.lib.mvs_allreduce_max_i64(self.ctx._h, self._h, ctypes.byref(v)))
        return v.value


def comm_library():
    """(path, version) of the RCCL the library's communicators use -- bound at run time; raises MvsError without one"""
    lib = load_library()
    buf = ctypes.create_string_buffer(4096)
    ver = _c.c_int()
    _check(lib.mvs_comm_library(buf, len(buf), ctypes.byref(ver)))
    return buf.value.decode("utf-8", "replace"), ver.value


def comm_unique_id():
    """rank 0: the 128-byte RCCL id to hand to the other ranks"""
    buf = ctypes.create_string_buffer(COMM_ID_BYTES)
    _check(load_library().mvs_comm_unique_id(buf))
    return buf.raw


class Context:
    """One device + one stream (mvs_ctx)."""

    def __init__(self, device=0, stream=None):
        self.lib = load_library()
        h = _P()
        _check(self.lib.mvs_ctx_create(int(device), ctypes.byref(h)))
        self._h = h
        self.device = device
        self._sets = weakref.WeakSet()   # sketch sets hold a pointer to the context: close them first
        self._comms = weakref.WeakSet()  # communicators likewise
        self._children = weakref.WeakSet()   # clusters, linkages, dereplications, hash sets, PCAs: after those two, before the context
        if stream is not None:
            self.set_stream(stream)

    def close(self):
        if getattr(self, "_h", None):
            for s in list(self._sets):
                s.close()
            for m in list(self._comms):
                m.close()
            for k in list(self._children):
                k.close()
            self.lib.mvs_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, stream):
        """stream: a torch.cuda.Stream or a raw hipStream_t value (0 = HIP's default stream);
        None switches back to the context's own non-blocking stream."""
        if stream is None:
            _check(self.lib.mvs_ctx_use_own_stream(self._h))
            return
        if hasattr(stream, "cuda_stream"):
            stream = stream.cuda_stream
        _check(self.lib.mvs_ctx_set_stream(self._h, _P(int(stream)) if int(stream) else None))

    def synchronize(self):
        _check(self.lib.mvs_ctx_synchronize(self._h))

    def comm_rccl(self, unique_id, rank, world):
        h = _P()
        _check(self.lib.mvs_comm_create(self._h, unique_id, int(rank), int(world), ctypes.byref(h)))
        return Comm(self, h)

    def comm_files(self, path_prefix, rank, world):
        h = _P()
        _check(self.lib.mvs_comm_create_files(self._h, path_prefix.encode(), int(rank), int(world), ctypes.byref(h)))
        return Comm(self, h)

    def comm_rendezvous(self, path_prefix, rank, world):
        """RCCL communicator whose ranks find each other under a path prefix (mvs_comm_create_rendezvous)"""
        h = _P()
        _check(self.lib.mvs_comm_create_rendezvous(self._h, path_prefix.encode(), int(rank), int(world), ctypes.byref(h)))
        return Comm(self, h)

    def set_option(self, name, value):
        """tuning / diagnostic switch of this context (include/mvs_hip.h lists them); never changes a result"""
        _check(self.lib.mvs_ctx_set_option(self._h, name.encode(), int(value)))

    def get_option(self, name):
        v = _c.c_int64()
        _check(self.lib.mvs_ctx_get_option(self._h, name.encode(), ctypes.byref(v)))
        return v.value

    def options(self, **kw):
        """`with ctx.options(pairwise_filter=0): ...` -- set, run, restore"""
        ctx = self

        class _Scope:
            def __enter__(self):
                self.old = {k: ctx.get_option(k) for k in kw}
                for k, v in kw.items():
                    ctx.set_option(k, v)
                return ctx

            def __exit__(self, *exc):
                for k, v in self.old.items():
                    ctx.set_option(k, v)
                return False
        return _Scope()

    def set_timing(self, enabled=True):
        _check(self.lib.mvs_ctx_set_timing(self._h, 1 if enabled else 0))

    def kernel_ms(self, which):
        ms = _c.c_float()
        _check(self.lib.mvs_ctx_kernel_ms(self._h, which, ctypes.byref(ms)))
        return ms.value

    def pairwise_candidates(self):
        """candidate pairs the last comparison's coarse filter passed to the exact re-check (0: exact kernel only)"""
        v = _c.c_int64()
        _check(self.lib.mvs_ctx_pairwise_candidates(self._h, ctypes.byref(v)))
        return v.value

    def pairwise_stats(self):
        """(candidates, flagged_tiles, filter_tiles) of the last two-stage comparison: pairs re-checked one by one, and how
        many of the filter's 256 x 256 tiles went to the exact kernel whole"""
        a, b, t = _c.c_int64(), _c.c_int64(), _c.c_int64()
        _check(self.lib.mvs_ctx_pairwise_stats(self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(t)))
        return a.value, b.value, t.value

    def derived_stats(self):
        """mvs_ctx_derived_stats: dict of the cumulative counts of whole builds (coarse_builds, coarse_fm_builds,
        planes_fm_builds) and of rows re-derived in place after a fill (coarse_rows_refreshed, planes_fm_rows_refreshed)"""
        v = [_c.c_int64() for _ in range(5)]
        _check(self.lib.mvs_ctx_derived_stats(self._h, *[ctypes.byref(x) for x in v]))
        return dict(zip(("coarse_builds", "coarse_rows_refreshed", "coarse_fm_builds", "planes_fm_builds",
                         "planes_fm_rows_refreshed"), (x.value for x in v)))

    # ---- projection ----
    def project_stats(self):
        """(units, cut_samples, slots, ny) of the last projection: the units of work it launched, the samples that consist of
        several of them, and the resident workgroups / workgroups per unit its plan was made with (slots 0: not balanced)"""
        u, k, s, y = _c.c_int64(), _c.c_int64(), _c.c_int(), _c.c_int()
        _check(self.lib.mvs_ctx_project_stats(self._h, ctypes.byref(u), ctypes.byref(k), ctypes.byref(s), ctypes.byref(y)))
        return u.value, k.value, s.value, y.value

    def project_csr(self, hashes, offsets, d, out=None):
        """hashes: uint64 numpy array or torch CUDA tensor (int64 view of the bits is accepted);
        offsets: host int64 array (n_samples+1).  Returns out (numpy unless `out` is given)."""
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        n = len(offsets) - 1
        if _is_torch(hashes):
            hp, hm, hk = _buf(hashes)
        else:
            hp, hm, hk = _buf(hashes, np.uint64)
        if out is None:
            out = np.empty((n, d), dtype=np.int32)
        op, om, ok = _buf(out, np.int32, writable=True)
        _check(self.lib.mvs_project_csr(self._h, hp, hm, offsets.ctypes.data, n, int(d), op, om))
        return out

    def project_csr_stats(self, hashes, offsets, d, out, sumsq):
        """project_csr into the device tensor `out`, filling the device int64 tensor `sumsq` with the exact
        sums of squares; returns the largest |v| (fused into the projection kernel for every sample that is
        a single unit of work; one pass over the rows of the others)."""
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        n = len(offsets) - 1
        hp, hm, hk = _buf(hashes) if _is_torch(hashes) else _buf(hashes, np.uint64)
        op, om, ok = _buf(out)
        sp, sm, sk = _buf(sumsq)
        if om != MEM_DEVICE or sm != MEM_DEVICE:
            raise ValueError("out and sumsq must be device buffers")
        m = _c.c_int64()
        _check(self.lib.mvs_project_csr_stats(self._h, hp, hm, offsets.ctypes.data, n, int(d), op, om, sp,
                                              ctypes.byref(m)))
        return m.value

    def sumsq(self, sketches, out=None):
        n, d = sketches.shape
        ip, im, ik = _buf(sketches, np.int32)
        if out is None:
            out = np.empty(n, dtype=np.int64)
        op, om, ok = _buf(out, np.int64, writable=True)
        _check(self.lib.mvs_sketch_sumsq(self._h, ip, im, n, d, op, om))
        return out

    def norms_sq_text(self, sumsq, d, out):
        """device int64 sums of squares -> device float64 squared norms as they come back from vector_norms.txt
        (6-significant-digit text round trip, exact); asynchronous on the context's stream."""
        ip, im, ik = _buf(sumsq, np.int64)
        op, om, ok = _buf(out, np.float64, writable=True)
        if im != MEM_DEVICE or om != MEM_DEVICE:
            raise ValueError("norms_sq_text works on device arrays")
        _check(self.lib.mvs_norms_sq_text(self._h, ip, int(sumsq.shape[0]), int(d), op))
        return out

    def stats(self, sketches, out=None):
        """-> (sumsq, max_abs): per-row exact sum of squares and the largest |v|, one pass."""
        n, d = sketches.shape
        ip, im, ik = _buf(sketches, np.int32)
        if out is None:
            out = np.empty(n, dtype=np.int64)
        op, om, ok = _buf(out, np.int64, writable=True)
        m = _c.c_int64()
        _check(self.lib.mvs_sketch_stats(self._h, ip, im, n, d, op, om, ctypes.byref(m)))
        return out, m.value

    def saturate_i16(self, sketches, out=None):
        ip, im, ik = _buf(sketches, np.int32)
        n_elems = int(np.prod(sketches.shape))
        if out is None:
            out = np.empty(tuple(sketches.shape), dtype=np.int16)
        op, om, ok = _buf(out, np.int16, writable=True)
        _check(self.lib.mvs_sketch_saturate_i16(self._h, ip, im, n_elems, op, om))
        return out

    # ---- pairwise ----
    @staticmethod
    def _elem_bytes(sketches):
        if _is_torch(sketches):
            return sketches.element_size()
        return np.asarray(sketches).dtype.itemsize

    def max_abs(self, sketches):
        eb = self._elem_bytes(sketches)
        p, m, k = _buf(sketches)
        out = _c.c_int64()
        _check(self.lib.mvs_sketch_max_abs(self._h, p, eb, m, int(np.prod(sketches.shape)), ctypes.byref(out)))
        return out.value

    def limb_geometry(self, n, d, limbs):
        n_alloc, d_pad, nbytes = _c.c_int64(), _c.c_int(), _c.c_size_t()
        _check(self.lib.mvs_limb_geometry(n, d, limbs, n_alloc, d_pad, nbytes))
        return n_alloc.value, d_pad.value, nbytes.value

    def limb_split(self, sketches, limbs, planes, d_pad, row_offset=0):
        n, d = sketches.shape
        eb = self._elem_bytes(sketches)
        p, m, k = _buf(sketches)
        pp, pm, pk = _buf(planes)
        if pm != MEM_DEVICE:
            raise ValueError("planes must be a device buffer")
        _check(self.lib.mvs_limb_split(self._h, p, eb, m, n, d, limbs, pp, d_pad, row_offset))

    def sketch_set(self, sketches, limbs=None):
        """limbs=None lets the library choose the limb code from max|v|; an explicit code (1..4 or
        LIMBS_K3) allocates and fills the planes with that scheme (the caller guarantees the range)."""
        n, d = sketches.shape
        eb = self._elem_bytes(sketches)
        if eb not in (2, 4):
            raise ValueError("sketches must be int32 or int16")
        p, m, k = _buf(sketches)
        h = _P()
        if limbs is None:
            _check(self.lib.mvs_sketch_set_create(self._h, p, eb, m, n, d, ctypes.byref(h)))
        else:
            _check(self.lib.mvs_sketch_set_alloc(self._h, n, d, int(limbs), ctypes.byref(h)))
            rc = self.lib.mvs_sketch_set_fill(h, p, eb, m, 0, n)
            if rc != MVS_OK:
                self.lib.mvs_sketch_set_destroy(h)
                _check(rc)
            self.synchronize()
        return SketchSet(self, h)

    def sketch_set_alloc(self, n, d, limbs):
        """zeroed planes for n samples with limb code `limbs`; fill row ranges with SketchSet.fill"""
        h = _P()
        _check(self.lib.mvs_sketch_set_alloc(self._h, int(n), int(d), int(limbs), ctypes.byref(h)))
        return SketchSet(self, h)

    def sketch_set_from_planes(self, planes, n, n_alloc, d, d_pad, limbs):
        pp, pm, pk = _buf(planes)
        if pm != MEM_DEVICE:
            raise ValueError("planes must be a device buffer")
        h = _P()
        _check(self.lib.mvs_sketch_set_from_planes(self._h, pp, n, n_alloc, d, d_pad, limbs, ctypes.byref(h)))
        return SketchSet(self, h, keep=planes)

    def pairwise_rows(self, sset, norms_sq, row_begin=0, row_end=None, keep_mode=KEEP_INT32, capacity=None,
                      cells_out=None):
        """Returns (cells, n_cells).  cells is a numpy structured array (CELL_DTYPE) unless a device
        buffer `cells_out` (torch int32 tensor of shape [capacity, 4]) is given.  Grows the host buffer
        and retries on MVS_E_CAPACITY."""
        if row_end is None:
            row_end = sset.n
        np_, nm, nk = _norms(norms_sq)
        count = _c.c_int64()
        if cells_out is not None:
            cp, cm, ck = _buf(cells_out)
            cap = cells_out.shape[0]
            rc = self.lib.mvs_pairwise_rows(self._h, sset._h, np_, nm, keep_mode, row_begin, row_end, cp, cap, cm,
                                            ctypes.byref(count))
            _check(rc)
            return cells_out, count.value
        cap = capacity if capacity is not None else max(1024, 64 * (row_end - row_begin))
        while True:
            cells = np.empty(cap, dtype=CELL_DTYPE)
            rc = self.lib.mvs_pairwise_rows(self._h, sset._h, np_, nm, keep_mode, row_begin, row_end,
                                            cells.ctypes.data, cap, MEM_HOST, ctypes.byref(count))
            if rc == MVS_E_CAPACITY and capacity is None:
                cap = count.value
                continue
            _check(rc)
            return cells[:count.value], count.value

    def pairwise_stream(self, sset, norms_sq, on_block=None, row_begin=0, row_end=None, keep_mode=KEEP_INT32,
                        device_budget_bytes=0):
        """mvs_pairwise_stream: the kept cells of rows [row_begin, row_end) in CSR pieces of whole rows, ascending.
        on_block(row_begin, row_end, row_ptr, col, q) is called per piece with numpy COPIES (q is uint8, or uint16 in the
        mismatched-norms case); a truthy return stops the comparison (MvsError MVS_E_ABORTED).  Without on_block the
        pieces are collected: returns (row_ptr int64 [rows + 1], col int32 [n], q [n], n)."""
        if row_end is None:
            row_end = sset.n
        np_, nm, nk = _norms(norms_sq)
        pieces = _RowBlockPieces(on_block)
        count = _c.c_int64()
        rc = self.lib.mvs_pairwise_stream(self._h, sset._h, np_, nm, keep_mode, int(row_begin), int(row_end),
                                          int(device_budget_bytes), pieces.cb, None, ctypes.byref(count))
        pieces.check(rc)
        if on_block is not None:
            return count.value
        got = pieces.join(row_begin, row_end, count.value)
        return got["row_ptr"], got["col"], got["q"] if got["q"] is not None else got["q16"], count.value

    def pairwise_stream_encoded(self, sset, norms_sq, row_begin=0, row_end=None, keep_mode=KEEP_INT32, device_budget_bytes=0):
        """mvs_pairwise_stream_encoded, pieces collected: returns dict(rows uint32 [R], first_col uint32 [R], offset uint64
        [R] into `bytes`, jac_bytes uint32 [R], bytes uint8 [B] = what the shard writer appends to matrix.bin, n_cells)"""
        if row_end is None:
            row_end = sset.n
        np_, nm, nk = _norms(norms_sq)
        pieces = _EncodedPieces()
        count = _c.c_int64()
        rc = self.lib.mvs_pairwise_stream_encoded(self._h, sset._h, np_, nm, keep_mode, int(row_begin), int(row_end),
                                                  int(device_budget_bytes), pieces.cb, None, ctypes.byref(count))
        pieces.check(rc)
        return pieces.join(row_begin, row_end, count.value)

    def _device_cells(self, cells):
        """-> (device pointer or None, number of cells, keepalive) of a sorted cell list: a torch int32 device tensor [m, 4]
        (row, col, dot, q) as cells_sort takes it, or a numpy CELL_DTYPE array, which is uploaded"""
        if not _is_torch(cells):
            import torch
            a = np.ascontiguousarray(cells)
            if a.dtype != CELL_DTYPE:
                raise ValueError("cells must be CELL_DTYPE records or a torch int32 device tensor [m, 4]")
            cells = torch.from_numpy(a.view("<i4").reshape(-1, 4)).to(torch.device("cuda", self.device))
        if str(cells.dtype) != "torch.int32" or cells.dim() != 2 or cells.shape[1] != 4:
            raise ValueError("cells must be int32 [m, 4]")
        cp, cm, ck = _buf(cells)
        if cm != MEM_DEVICE:
            raise ValueError("cells must be a device buffer")
        return (_P(cp) if cells.shape[0] else None), int(cells.shape[0]), ck

    def cells_stream(self, cells, row_begin, row_end):
        """mvs_cells_stream, pieces collected: rows [row_begin, row_end) of a cell list ordered by (row, col) as CSR arrays.
        cells: torch int32 device tensor [m, 4] (row, col, dot, q) or a numpy CELL_DTYPE array (uploaded).  Returns
        dict(row_ptr int64 [rows + 1], col int32 [n], q uint8 [n] or None, q16 uint16 [n] or None -- the one the pieces came
        with --, n_cells, pieces)."""
        cp, m, _keepalive = self._device_cells(cells)      # holds the uploaded tensor until the call has returned
        pieces = _RowBlockPieces(None)
        count = _c.c_int64()
        rc = self.lib.mvs_cells_stream(self._h, cp, m, int(row_begin), int(row_end), pieces.cb, None, ctypes.byref(count))
        pieces.check(rc)
        return pieces.join(row_begin, row_end, count.value)

    def cells_stream_encoded(self, cells, row_begin, row_end):
        """mvs_cells_stream_encoded, pieces collected: the shard records of rows [row_begin, row_end) of a cell list ordered
        by (row, col); cells as for cells_stream.  Returns the dict pairwise_stream_encoded returns."""
        cp, m, _keepalive = self._device_cells(cells)      # holds the uploaded tensor until the call has returned
        pieces = _EncodedPieces()
        count = _c.c_int64()
        rc = self.lib.mvs_cells_stream_encoded(self._h, cp, m, int(row_begin), int(row_end), pieces.cb, None, ctypes.byref(count))
        pieces.check(rc)
        return pieces.join(row_begin, row_end, count.value)

    def stream_stats(self):
        """what the last pairwise_stream did: dict(kernel_ms, bytes, row_blocks, pieces, two_stage: 0 exact kernel, 1 two-stage as one list, 2 two-stage through the dense byte matrix)"""
        k, b, r, p_, t = _c.c_double(), _c.c_int64(), _c.c_int64(), _c.c_int64(), _c.c_int()
        _check(self.lib.mvs_ctx_stream_stats(self._h, ctypes.byref(k), ctypes.byref(b), ctypes.byref(r), ctypes.byref(p_),
                                             ctypes.byref(t)))
        return {"kernel_ms": k.value, "bytes": b.value, "row_blocks": r.value, "pieces": p_.value, "two_stage": int(t.value)}

    def stream_dense_stats(self):
        """mvs_ctx_stream_dense_stats: the route the last stream call's row blocks took -- dict(dense_blocks: delivered out
        of the dense byte matrix, spec_blocks: row passes queued with buffers sized from the blocks before, spec_redone: of
        those, done again because the sizes did not hold, list_fallbacks: dense blocks with a q a byte cannot hold, after
        which the rows went through packed lists)"""
        v = [_c.c_int64() for _ in range(4)]
        _check(self.lib.mvs_ctx_stream_dense_stats(self._h, *[ctypes.byref(x) for x in v]))
        return dict(zip(("dense_blocks", "spec_blocks", "spec_redone", "list_fallbacks"), (x.value for x in v)))

    def pairwise_block(self, sset, norms_sq, row_begin, row_end, col_begin, col_end, flags, cells, n_cells,
                       keep_mode=KEEP_INT32):
        """Append the kept cells of one block to the device buffer `cells` ([capacity, 4] int32) at index
        n_cells; returns the new count."""
        np_, nm, nk = _buf(norms_sq)
        cp, cm, ck = _buf(cells)
        if nm != MEM_DEVICE or cm != MEM_DEVICE:
            raise ValueError("norms_sq and cells must be device buffers")
        count = _c.c_int64(int(n_cells))
        rc = self.lib.mvs_pairwise_block(self._h, sset._h, np_, keep_mode, row_begin, row_end, col_begin, col_end,
                                         flags, cp, cells.shape[0], ctypes.byref(count))
        if rc == MVS_E_CAPACITY:
            raise MvsError(rc, self.lib.mvs_last_error().decode("utf-8", "replace"), needed=count.value)
        _check(rc)
        return count.value

    def search_block(self, sset, norms_sq, jaccard_min, row_begin, row_end, col_begin, col_end, cells):
        """pairs (query row, database column) with Jaccard estimate > jaccard_min -> number of hits written to
        the device buffer `cells`, sorted by (row, col)"""
        np_, nm, nk = _buf(norms_sq)
        cp, cm, ck = _buf(cells)
        if nm != MEM_DEVICE or cm != MEM_DEVICE:
            raise ValueError("norms_sq and cells must be device buffers")
        count = _c.c_int64()
        rc = self.lib.mvs_search_block(self._h, sset._h, np_, float(jaccard_min), row_begin, row_end, col_begin,
                                       col_end, cp, cells.shape[0], ctypes.byref(count))
        if rc == MVS_E_CAPACITY:       # count = the hits there are: the caller can come back with exactly that room
            raise MvsError(rc, self.lib.mvs_last_error().decode("utf-8", "replace"), needed=count.value)
        _check(rc)
        return count.value

    # ---- block plans (include/mvs_hip.h "block plans"): a rank's share of the symmetric multi-rank schedule ----
    def attach_derived(self, sset, coarse_fm, row_stats):
        """the filter's inputs of `sset` live in these device buffers from now on (n_alloc * d_pad bytes, n_alloc * 16 bytes)"""
        cp, cm, ck = _buf(coarse_fm)
        rp, rm, rk = _buf(row_stats)
        if cm != MEM_DEVICE or rm != MEM_DEVICE:
            raise ValueError("device buffers required")
        _check(self.lib.mvs_sketch_set_attach_derived(sset._h, cp, rp))
        sset._derived = (coarse_fm, row_stats)

    def prepare_rows(self, sset, row_first, row_count):
        _check(self.lib.mvs_sketch_set_prepare_rows(self._h, sset._h, int(row_first), int(row_count)))

    def recode_rows(self, sset, sketches, row_first, row_count):
        """limb planes + filter inputs of rows [row_first, row_first + row_count) in one pass: the first len(sketches) of them
        from `sketches` (device [n, d]; None: none), the rest zero rows"""
        n = 0 if sketches is None else sketches.shape[0]
        sp, sm, sk = _buf(sketches)
        if n and sm != MEM_DEVICE:
            raise ValueError("sketches must be a device buffer")
        _check(self.lib.mvs_sketch_set_recode_rows(self._h, sset._h, sp, self._elem_bytes(sketches) if n else 4, n, int(row_first),
                                                   int(row_count)))

    def planes_from_wire(self, sset, lo_wire, row_first, row_count):
        """limb planes of rows [row_first, row_first + row_count) from their low limbs (lo_wire: device bytes, row r at
        r * d_pad) and the attached coarse plane / statistics (mvs_sketch_set_planes_from_wire)"""
        lp, lm, lk = _buf(lo_wire)
        if lm != MEM_DEVICE:
            raise ValueError("the wire buffer must be a device buffer")
        _check(self.lib.mvs_sketch_set_planes_from_wire(self._h, sset._h, lp, int(row_first), int(row_count)))

    def plan_rows_ready(self, row_begin, row_end):
        """statistics and norms of these rows are in place: their filter constants in one launch (mvs_plan_rows_ready)"""
        _check(self.lib.mvs_plan_rows_ready(self._h, int(row_begin), int(row_end)))

    def plan_wire(self, lo_wire):
        """the plan in progress rebuilds the limb planes of the foreign rows its second half reads from lo_wire (mvs_plan_wire)"""
        lp, lm, lk = _buf(lo_wire)
        if lm != MEM_DEVICE:
            raise ValueError("the wire buffer must be a device buffer")
        _check(self.lib.mvs_plan_wire(self._h, lp))

    def plan_begin(self, sset, norms_sq, frame_begin, frame_end, mirror_outside, cells, keep_mode=KEEP_INT32):
        np_, nm, nk = _buf(norms_sq)
        cp, cm, ck = _buf(cells)
        if nm != MEM_DEVICE or cm != MEM_DEVICE:
            raise ValueError("norms_sq and cells must be device buffers")
        _check(self.lib.mvs_plan_begin(self._h, sset._h, np_, keep_mode, int(frame_begin), int(frame_end),
                                       PLAN_MIRROR_OUTSIDE if mirror_outside else 0, cp, cells.shape[0]))

    def plan_filter(self, blocks):
        """blocks: [(row_begin, row_end, col_begin, col_end)] -> ONE filter launch (asynchronous)"""
        arr = (_c.c_int64 * (4 * len(blocks)))(*[int(x) for b in blocks for x in b[:4]])
        _check(self.lib.mvs_plan_filter(self._h, arr, len(blocks)))

    def plan_finish(self):
        """re-check + flagged tiles; -> device address of the running cell count"""
        p = _P()
        _check(self.lib.mvs_plan_finish(self._h, ctypes.byref(p)))
        return p.value

    def plan_stats(self):
        ms = (_c.c_double * 4)()
        cnt = (_c.c_int64 * 6)()
        _check(self.lib.mvs_plan_stats(self._h, ms, cnt))
        return {"filter_ms": ms[0], "recheck_ms": ms[1], "tiles_ms": ms[2], "span_ms": ms[3], "candidates": cnt[0],
                "flagged_tiles": cnt[1], "filter_tiles": cnt[2], "filter_launches": cnt[3], "exact_mode": bool(cnt[4] & 1),
                "speculated": bool(cnt[4] & 2), "stale": bool(cnt[4] & 4), "d_pad": cnt[5]}

    def cells_route(self, raw, d_n_raw, block_pad, block_rows, n_total, own_begin, own_end, own_out, d_own_count, send,
                    foreign_capacity, status=0, max_abs=0):
        """d_n_raw: device ADDRESS (int) of the cell count (plan_finish); d_own_count: device tensor of one int64 / uint64"""
        rp, rm, rk = _buf(raw)
        op, om, ok = _buf(own_out)
        cp, cm, ck = _buf(d_own_count)
        sp, sm, sk = _buf(send)
        if rm != MEM_DEVICE or om != MEM_DEVICE or cm != MEM_DEVICE or (send is not None and sm != MEM_DEVICE):
            raise ValueError("device buffers required")
        _check(self.lib.mvs_cells_route(self._h, rp, _P(int(d_n_raw)), raw.shape[0], int(block_pad), int(block_rows), int(n_total),
                                        int(own_begin), int(own_end), op, own_out.shape[0], cp, sp, int(foreign_capacity),
                                        int(status), int(max_abs)))

    def cells_collect(self, recv, world, rank, foreign_capacity, own_begin, own_end, own_out, d_own_count):
        rp, rm, rk = _buf(recv)
        op, om, ok = _buf(own_out)
        cp, cm, ck = _buf(d_own_count)
        _check(self.lib.mvs_cells_collect(self._h, rp, int(world), int(rank), int(foreign_capacity), int(own_begin), int(own_end),
                                          op, own_out.shape[0], cp))

    def cells_report(self, recv, world, foreign_capacity, own_rows, d_own_count):
        """-> (cells of this shard, [(foreign cells, status, max_abs, raw cells, raw capacity)] per rank, most cells in one
        row); synchronises"""
        rp, rm, rk = _buf(recv)
        cp, cm, ck = _buf(d_own_count)
        out = (_c.c_int64 * (2 + 5 * world))()
        _check(self.lib.mvs_cells_report(self._h, rp, int(world), int(foreign_capacity), int(own_rows), cp, out))
        return out[0], [tuple(out[1 + 5 * r:6 + 5 * r]) for r in range(world)], out[1 + 5 * world]

    def cells_sort_rows(self, cells_in, n, own_begin, own_end, d_own_count, cells_out):
        ip, im, ik = _buf(cells_in)
        op, om, ok = _buf(cells_out)
        cp, cm, ck = _buf(d_own_count)
        _check(self.lib.mvs_cells_sort_rows(self._h, ip, int(n), int(own_begin), int(own_end), cp, op))

    def cells_sort_rows_ahead(self, cells_in, own_begin, own_end, d_own_count, cells_out):
        """the row-bucket sort queued before the report's read-back: the count is the one on the device, both buffers' sizes bound it"""
        ip, im, ik = _buf(cells_in)
        op, om, ok = _buf(cells_out)
        cp, cm, ck = _buf(d_own_count)
        _check(self.lib.mvs_cells_sort_rows_ahead(self._h, ip, int(cells_in.shape[0]), int(own_begin), int(own_end), cp, op,
                                                  int(cells_out.shape[0])))

    def cells_sort(self, cells_in, n, cells_out):
        ip, im, ik = _buf(cells_in)
        op, om, ok = _buf(cells_out)
        if im != MEM_DEVICE or om != MEM_DEVICE:
            raise ValueError("device buffers required")
        _check(self.lib.mvs_cells_sort(self._h, ip, int(n), op))

    def pairwise_topk(self, sset, norms_sq, k, row_begin=0, row_end=None, col_begin=0, col_end=None, exclude_self=True,
                      cells_out=None):
        """mvs_pairwise_topk: per row of [row_begin, row_end) the k columns of [col_begin, col_end) with the highest Jaccard
        estimate (ties: the smaller column; NaN never), each row's cells in ascending column order.  Returns a structured
        CELL_DTYPE array sorted by (row, col), or -- with a device buffer `cells_out` (torch int32 tensor [rows * k, 4]) --
        (cells_out, n_cells)."""
        if row_end is None:
            row_end = sset.n
        if col_end is None:
            col_end = sset.n
        np_, nm, nk = _norms(norms_sq)
        flags = TOPK_EXCLUDE_SELF if exclude_self else 0
        count = _c.c_int64()
        if cells_out is not None:
            cp, cm, ck = _buf(cells_out)
            _check(self.lib.mvs_pairwise_topk(self._h, sset._h, np_, nm, int(k), int(row_begin), int(row_end), int(col_begin),
                                              int(col_end), flags, cp, cm, ctypes.byref(count)))
            return cells_out, count.value
        cells = np.empty(max(1, (row_end - row_begin) * max(int(k), 0)), dtype=CELL_DTYPE)
        _check(self.lib.mvs_pairwise_topk(self._h, sset._h, np_, nm, int(k), int(row_begin), int(row_end), int(col_begin),
                                          int(col_end), flags, cells.ctypes.data, MEM_HOST, ctypes.byref(count)))
        return cells[:count.value]

    def topk_stats(self):
        """-> dict of the last pairwise_topk: dots_ms / select_ms (kernel times over its row blocks, timing on), row_blocks,
        block_rows"""
        a, b = _c.c_double(), _c.c_double()
        n, r = _c.c_int64(), _c.c_int64()
        _check(self.lib.mvs_ctx_topk_stats(self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(n), ctypes.byref(r)))
        return {"dots_ms": a.value, "select_ms": b.value, "row_blocks": n.value, "block_rows": r.value}

    def pairwise_contain(self, sset, norms_sq, min_containment, slack=0.0, mode="row", row_begin=0, row_end=None, col_begin=0,
                         col_end=None, cells_out=None):
        """mvs_pairwise_contain: the cells (row, col), row != col, whose estimated containment of the row's sample in the
        column's exceeds min_containment (0 < c < 1) by more than `slack` standard errors (include/mvs_hip.h states the rule);
        mode "row" keeps the directed cells, "max" a cell that passes in either direction.  Returns a structured CELL_DTYPE
        array sorted by (row, col) -- q is the quantised containment estimate -- or, with a device buffer `cells_out` (torch
        int32 tensor [capacity, 4]), (cells_out, n_cells); a buffer that is too small raises MvsError with `needed` set."""
        if mode not in ("row", "max"):
            raise ValueError("mode must be 'row' or 'max'")
        if row_end is None:
            row_end = sset.n
        if col_end is None:
            col_end = sset.n
        np_, nm, nk = _norms(norms_sq)
        flags = CONTAIN_MAX if mode == "max" else CONTAIN_ROW
        count = _c.c_int64()

        def call(ptr, mem, capacity):
            rc = self.lib.mvs_pairwise_contain(self._h, sset._h, np_, nm, float(min_containment), float(slack), flags,
                                               int(row_begin), int(row_end), int(col_begin), int(col_end), ptr, mem,
                                               int(capacity), ctypes.byref(count))
            if rc == MVS_E_CAPACITY:
                raise MvsError(rc, self.lib.mvs_last_error().decode("utf-8", "replace"), needed=count.value)
            _check(rc)

        if cells_out is not None:
            cp, cm, ck = _buf(cells_out)
            call(cp, cm, cells_out.shape[0])
            return cells_out, count.value
        capacity = max(1024, 16 * max(0, int(row_end) - int(row_begin)))
        for attempt in range(2):
            cells = np.empty(capacity, dtype=CELL_DTYPE)
            try:
                call(cells.ctypes.data, MEM_HOST, capacity)
                break
            except MvsError as e:
                if e.code != MVS_E_CAPACITY or attempt:
                    raise
                capacity = int(e.needed)
        return cells[:count.value]

    def contain_stats(self):
        """-> dict of the last pairwise_contain: dots_ms / select_ms (kernel times over its row blocks, timing on), row_blocks,
        block_rows"""
        a, b = _c.c_double(), _c.c_double()
        n, r = _c.c_int64(), _c.c_int64()
        _check(self.lib.mvs_ctx_contain_stats(self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(n), ctypes.byref(r)))
        return {"dots_ms": a.value, "select_ms": b.value, "row_blocks": n.value, "block_rows": r.value}

    def pairwise_levels(self, sset, norms_sq, levels, row_begin=0, row_end=None, col_begin=0, col_end=None, degrees_out=None):
        """mvs_pairwise_levels: for every row of [row_begin, row_end) the number of columns of [col_begin, col_end), self
        excluded, it is linked to at each of the strictly ascending Jaccard `levels` (1 .. 64 values in (0, 1);
        include/mvs_hip.h states the rule: the link rule of the clustering, per level).  Returns (degrees int32 [rows, m],
        totals int64 [m]), totals[l] = the rows' sum at level l.  `degrees_out`: a torch device tensor (int32 [rows, m]) or a
        numpy int32 array to fill and return instead of a new array; False: totals only, (None, totals)."""
        if row_end is None:
            row_end = sset.n
        if col_end is None:
            col_end = sset.n
        np_, nm, nk = _norms(norms_sq)
        lv = np.ascontiguousarray(levels, dtype=np.float64).reshape(-1)
        m = len(lv)
        rows = max(0, int(row_end) - int(row_begin))
        totals = np.zeros(max(m, 1), dtype=np.int64)
        if degrees_out is False:
            degrees, dp, dm = None, None, MEM_HOST
        elif degrees_out is None:
            degrees = np.zeros((rows, m), dtype=np.int32)
            dp, dm = degrees.ctypes.data, MEM_HOST
        else:
            if tuple(degrees_out.shape) != (rows, m):
                raise ValueError("degrees_out must have shape (%d, %d)" % (rows, m))
            if _is_torch(degrees_out):
                import torch
                if degrees_out.dtype != torch.int32:
                    raise ValueError("degrees_out must be an int32 tensor")
            degrees = degrees_out
            dp, dm, dk = _buf(degrees_out, np.int32, writable=True)
        _check(self.lib.mvs_pairwise_levels(self._h, sset._h, np_, nm, lv.ctypes.data, m, int(row_begin), int(row_end), int(col_begin),
                                            int(col_end), dp, dm, totals.ctypes.data))
        return degrees, totals[:m]

    def levels_stats(self):
        """-> dict of the last pairwise_levels: dots_ms / count_ms (kernel times over its row blocks, timing on), row_blocks,
        block_rows"""
        a, b = _c.c_double(), _c.c_double()
        n, r = _c.c_int64(), _c.c_int64()
        _check(self.lib.mvs_ctx_levels_stats(self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(n), ctypes.byref(r)))
        return {"dots_ms": a.value, "count_ms": b.value, "row_blocks": n.value, "block_rows": r.value}

    # ---- ordination (include/mvs_hip.h "ordination") ----
    def sketch_moments(self, sset, row_begin=0, row_end=None):
        """mvs_sketch_moments: the exact moments of rows [row_begin, row_end) over the sample axis -> (gram int64 [d, d],
        col_sums int64 [d]); gram[a, b] = sum_i x[i, a] x[i, b]"""
        if row_end is None:
            row_end = sset.n
        gram = np.empty((sset.d, sset.d), dtype=np.int64)
        sums = np.empty(sset.d, dtype=np.int64)
        _check(self.lib.mvs_sketch_moments(self._h, sset._h, int(row_begin), int(row_end), gram.ctypes.data, sums.ctypes.data, MEM_HOST))
        return gram, sums

    def pca(self, sset, components, row_begin=0, row_end=None, tol=1e-10, max_iters=300):
        """mvs_pca_fit: the `components` leading principal axes of rows [row_begin, row_end) of `sset` -> Pca.  A fit that did
        not reach `tol` within `max_iters` iterations still returns (Pca.converged is False)."""
        if row_end is None:
            row_end = sset.n
        h = _P()
        _check(self.lib.mvs_pca_fit(self._h, sset._h, int(row_begin), int(row_end), int(components), float(tol), int(max_iters),
                                    ctypes.byref(h)))
        return Pca(self, h)

    def pca_stats(self):
        """-> dict of the last sketch_moments / pca / Pca.transform: gram_ms, eigen_ms, scores_ms (timing on), slabs, iterations"""
        a, b, s = _c.c_double(), _c.c_double(), _c.c_double()
        n, r = _c.c_int64(), _c.c_int64()
        _check(self.lib.mvs_ctx_pca_stats(self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(s), ctypes.byref(n), ctypes.byref(r)))
        return {"gram_ms": a.value, "eigen_ms": b.value, "scores_ms": s.value, "slabs": n.value, "iterations": r.value}

    # ---- principal coordinates of the Jaccard estimates (include/mvs_hip.h "principal coordinates") ----
    def jaccard_apply(self, sset, norms_sq, X, rows=None, cols=None, floor=0.0):
        """mvs_jaccard_apply: Y = K X over `rows` x `cols` (each a (begin, end) pair, default every sample), K the clamped
        Jaccard estimates above `floor` with a unit diagonal (include/mvs_hip.h states the rule), never stored.  X: float64
        [cols, b] (or [cols]), 1 <= b <= 128 -> float64 [rows, b] (or [rows])."""
        rb, re = (0, sset.n) if rows is None else rows
        cb, ce = (0, sset.n) if cols is None else cols
        np_, nm, nk = _norms(norms_sq)
        x = np.ascontiguousarray(X, dtype=np.float64)
        flat = x.ndim == 1
        if flat:
            x = x.reshape(-1, 1)
        if x.ndim != 2 or x.shape[0] != max(0, int(ce) - int(cb)):
            raise ValueError("X must have one row per column of the range")
        b = x.shape[1]
        out = np.empty((max(0, int(re) - int(rb)), b), dtype=np.float64)
        _check(self.lib.mvs_jaccard_apply(self._h, sset._h, np_, nm, float(floor), int(rb), int(re), int(cb), int(ce), x.ctypes.data, b,
                                          MEM_HOST, out.ctypes.data, MEM_HOST))
        return out[:, 0] if flat else out

    def pcoa(self, sset, norms_sq, components, rows=None, floor=0.0, tol=1e-10, max_iters=300):
        """mvs_pcoa_fit: principal coordinates of the Jaccard estimates of `rows` = (begin, end) of `sset` (default all) ->
        Pcoa.  A fit that did not reach `tol` within `max_iters` iterations still returns (Pcoa.converged is False)."""
        rb, re = (0, sset.n) if rows is None else rows
        np_, nm, nk = _norms(norms_sq)
        h = _P()
        _check(self.lib.mvs_pcoa_fit(self._h, sset._h, np_, nm, int(rb), int(re), int(components), float(floor), float(tol), int(max_iters),
                                     ctypes.byref(h)))
        return Pcoa(self, h, sset, nk if nk is not None else norms_sq)

    def pcoa_stats(self):
        """-> dict of the last jaccard_apply / pcoa / Pcoa.transform: dots_ms, apply_ms (kernel times over passes and row blocks),
        eigen_ms (the whole solver, host work included; timing on), passes, row_blocks, block_rows"""
        a, b, e = _c.c_double(), _c.c_double(), _c.c_double()
        n, r, k = _c.c_int64(), _c.c_int64(), _c.c_int64()
        _check(self.lib.mvs_ctx_pcoa_stats(self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(e), ctypes.byref(n), ctypes.byref(r),
                                           ctypes.byref(k)))
        return {"dots_ms": a.value, "apply_ms": b.value, "eigen_ms": e.value, "passes": n.value, "row_blocks": r.value, "block_rows": k.value}

    # ---- PERMANOVA on the Jaccard estimates (include/mvs_hip.h "PERMANOVA") ----
    def group_sums(self, sset, norms_sq, labels, groups, rows=None, floor=0.0):
        """mvs_group_sums: labels uint8 [slots, m] (or [m]), every value < groups, m the size of `rows` = (begin, end) of `sset`
        (default all) -> (sums, sizes): sums an object array [slots, groups] of Python ints, the within-group sums of the
        quantised squared distances w over unordered pairs; sizes int64 [slots, groups]."""
        rb, re = (0, sset.n) if rows is None else rows
        m = max(0, int(re) - int(rb))
        lab = np.ascontiguousarray(labels, dtype=np.uint8)
        if lab.ndim == 1:
            lab = lab.reshape(1, -1)
        if lab.ndim != 2 or lab.shape[1] != m:
            raise ValueError("labels must have one column per row of the range")
        slots, groups = lab.shape[0], int(groups)
        np_, nm, nk = _norms(norms_sq)
        cells = max(0, slots) * max(0, groups)
        lo, hi = np.zeros(cells, dtype=np.uint64), np.zeros(cells, dtype=np.uint64)
        sizes = np.zeros(cells, dtype=np.int64)
        _check(self.lib.mvs_group_sums(self._h, sset._h, np_, nm, float(floor), int(rb), int(re), lab.ctypes.data, slots, groups,
                                       lo.ctypes.data, hi.ctypes.data, sizes.ctypes.data))
        sums = np.array([(int(h) << 64) | int(l) for l, h in zip(lo.tolist(), hi.tolist())], dtype=object)
        return sums.reshape(slots, groups), sizes.reshape(slots, groups)

    def permanova(self, sset, norms_sq, labels, permutations=999, seed=0, rows=None, floor=0.0):
        """mvs_permanova: labels uint8 [m], one group id per sample of `rows` = (begin, end) of `sset` (default all); the
        number of group ids is max(labels) + 1 -> Permanova"""
        rb, re = (0, sset.n) if rows is None else rows
        m = max(0, int(re) - int(rb))
        lab = np.ascontiguousarray(labels, dtype=np.uint8)
        if lab.ndim != 1 or len(lab) != m:
            raise ValueError("labels must have one entry per row of the range")
        groups = int(lab.max()) + 1 if m else 1
        np_, nm, nk = _norms(norms_sq)
        res = PermanovaResult()
        sizes = np.zeros(groups, dtype=np.int64)
        mean = np.zeros(groups, dtype=np.float64)
        perm_f = np.zeros(max(0, int(permutations)), dtype=np.float64)
        _check(self.lib.mvs_permanova(self._h, sset._h, np_, nm, float(floor), int(rb), int(re), lab.ctypes.data, groups, int(permutations),
                                      int(seed) & (2 ** 64 - 1), ctypes.byref(res), sizes.ctypes.data, mean.ctypes.data, perm_f.ctypes.data))
        return Permanova(res, sizes, mean, perm_f)

    def groups_stats(self):
        """-> dict of the last group_sums / permanova: dots_ms, quantise_ms, sums_ms (kernel times over its row blocks, timing
        on), row_blocks, block_rows, slots"""
        a, b, e = _c.c_double(), _c.c_double(), _c.c_double()
        n, r, k = _c.c_int64(), _c.c_int64(), _c.c_int64()
        _check(self.lib.mvs_ctx_groups_stats(self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(e), ctypes.byref(n), ctypes.byref(r),
                                             ctypes.byref(k)))
        return {"dots_ms": a.value, "quantise_ms": b.value, "sums_ms": e.value, "row_blocks": n.value, "block_rows": r.value, "slots": k.value}

    # ---- the quality of a labelling on the Jaccard estimates (include/mvs_hip.h "Labelling quality") ----
    def label_sums(self, sset, norms_sq, labels, groups=None, rows=None, floor=0.0):
        """mvs_label_sums: labels int32 [m] in [-1, groups), -1 = unlabelled, m the size of `rows` = (begin, end) of `sset` (default
        all); groups defaults to max(labels) + 1 -> (own_sum uint64 [m], near_group int32 [m], near_sum uint64 [m], sizes int64
        [groups]): the sum of the quantised distances w to the sample's own group, the other group with the smallest mean
        distance (-1: none) and the sum over that group"""
        rb, re = (0, sset.n) if rows is None else rows
        m = max(0, int(re) - int(rb))
        lab = _labels(labels, m)
        groups = (max(1, int(lab.max()) + 1) if m else 1) if groups is None else int(groups)
        np_, nm, nk = _norms(norms_sq)
        own, nsum = np.zeros(m, dtype=np.uint64), np.zeros(m, dtype=np.uint64)
        near = np.full(m, -1, dtype=np.int32)
        sizes = np.zeros(max(0, groups), dtype=np.int64)
        _check(self.lib.mvs_label_sums(self._h, sset._h, np_, nm, float(floor), int(rb), int(re), lab.ctypes.data, groups, own.ctypes.data,
                                       near.ctypes.data, nsum.ctypes.data, sizes.ctypes.data))
        return own, near, nsum, sizes

    def silhouette(self, sset, norms_sq, labels, rows=None, floor=0.0):
        """mvs_silhouette: labels int32 [m], one group id per sample of `rows` = (begin, end) of `sset` (default all), -1 =
        unlabelled; the number of group ids is max(labels) + 1 -> Silhouette"""
        rb, re = (0, sset.n) if rows is None else rows
        m = max(0, int(re) - int(rb))
        lab = _labels(labels, m)
        groups = max(1, int(lab.max()) + 1) if m else 1
        np_, nm, nk = _norms(norms_sq)
        res = SilhouetteResult()
        s, a, b, c2 = (np.zeros(m, dtype=np.float64) for _ in range(4))
        near = np.full(m, -1, dtype=np.int32)
        sizes, med = np.zeros(groups, dtype=np.int64), np.zeros(groups, dtype=np.int64)
        gm, gw, gd = (np.zeros(groups, dtype=np.float64) for _ in range(3))
        _check(self.lib.mvs_silhouette(self._h, sset._h, np_, nm, float(floor), int(rb), int(re), lab.ctypes.data, groups, ctypes.byref(res),
                                       sizes.ctypes.data, near.ctypes.data, s.ctypes.data, a.ctypes.data, b.ctypes.data, c2.ctypes.data,
                                       gm.ctypes.data, gw.ctypes.data, gd.ctypes.data, med.ctypes.data))
        return Silhouette(res, s, a, b, near, c2, sizes, gm, gw, gd, med)

    def label_stats(self):
        """-> dict of the last label_sums / silhouette: dots_ms, reduce_ms (kernel times over its row blocks), gather_ms (timing
        on), row_blocks, block_rows"""
        a, b, e = _c.c_double(), _c.c_double(), _c.c_double()
        n, r = _c.c_int64(), _c.c_int64()
        _check(self.lib.mvs_ctx_label_stats(self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(e), ctypes.byref(n), ctypes.byref(r)))
        return {"dots_ms": a.value, "reduce_ms": b.value, "gather_ms": e.value, "row_blocks": n.value, "block_rows": r.value}

    # ---- average and complete linkage (include/mvs_hip.h "Average and complete linkage") ----
    def hclust(self, sset, norms_sq, method="average", floor=0.0, rows=None):
        """mvs_hclust: the agglomerative tree of the Jaccard distances of `rows` = (begin, end) of `sset` (default all), method
        'average' (UPGMA) or 'complete' -> Hclust; slot i is sample begin + i"""
        rb, re = (0, sset.n) if rows is None else rows
        m = max(0, int(re) - int(rb))
        np_, nm, nk = _norms(norms_sq)
        merges = np.zeros(max(0, m - 1), dtype=HMERGE_DTYPE)
        rounds = _c.c_int64()
        meth = _hclust_method(method)
        _check(self.lib.mvs_hclust(self._h, sset._h, np_, nm, float(floor), int(rb), int(re), meth, merges.ctypes.data, ctypes.byref(rounds)))
        return Hclust(m, meth, merges, rounds.value)

    def hclust_weights(self, w, method="average"):
        """mvs_hclust_weights: w uint32 [m, m] <= 2^30, symmetric off the diagonal (numpy, or a torch tensor of 32-bit integers on
        the host or the device) -> Hclust"""
        if not _is_torch(w):
            w = np.ascontiguousarray(w, dtype=np.uint32)
        if w.ndim != 2 or w.shape[0] != w.shape[1]:
            raise ValueError("w must be square")
        m = int(w.shape[0])
        wp, wm, wk = _buf(w)
        merges = np.zeros(max(0, m - 1), dtype=HMERGE_DTYPE)
        rounds = _c.c_int64()
        meth = _hclust_method(method)
        _check(self.lib.mvs_hclust_weights(self._h, wp, wm, m, meth, merges.ctypes.data, ctypes.byref(rounds)))
        return Hclust(m, meth, merges, rounds.value)

    def hclust_sums(self, sums, sizes=None, method="average"):
        """mvs_hclust_sums: sums uint64 [m, m], symmetric off the diagonal, every entry <= n_a n_b 2^30 (numpy, or a torch tensor
        of 64-bit integers); sizes int32 [m] >= 1 with a total <= 2^17, None = ones -> Hclust"""
        if not _is_torch(sums):
            sums = np.ascontiguousarray(sums, dtype=np.uint64)
        if sums.ndim != 2 or sums.shape[0] != sums.shape[1]:
            raise ValueError("sums must be square")
        m = int(sums.shape[0])
        sp, sm, sk = _buf(sums)
        zp = None
        if sizes is not None:
            sizes = np.ascontiguousarray(sizes, dtype=np.int32)
            if sizes.ndim != 1 or len(sizes) != m:
                raise ValueError("sizes must have one entry per slot")
            zp = sizes.ctypes.data
        merges = np.zeros(max(0, m - 1), dtype=HMERGE_DTYPE)
        rounds = _c.c_int64()
        meth = _hclust_method(method)
        _check(self.lib.mvs_hclust_sums(self._h, sp, sm, zp, m, meth, merges.ctypes.data, ctypes.byref(rounds)))
        return Hclust(m, meth, merges, rounds.value)

    def hclust_stats(self):
        """-> dict of the last hclust / hclust_weights / hclust_sums: dots_ms, fill_ms (kernel times over the row blocks),
        nearest_ms, merge_ms, compact_ms (over the rounds; timing on), rounds, row_scans, bytes_scanned, compactions"""
        d = [_c.c_double() for _ in range(5)]
        n = [_c.c_int64() for _ in range(4)]
        _check(self.lib.mvs_ctx_hclust_stats(self._h, *[ctypes.byref(x) for x in d + n]))
        names = ("dots_ms", "fill_ms", "nearest_ms", "merge_ms", "compact_ms", "rounds", "row_scans", "bytes_scanned", "compactions")
        return {k: x.value for k, x in zip(names, d + n)}

    # ---- modularity communities (include/mvs_hip.h "Communities") ----
    def community_graph(self, n, d=0, norms_sq=None, floor=0.05):
        """-> CommunityGraph: an empty graph over n samples; norms_sq, d and floor decide the weight of a fed cell (None: the graph
        takes raw edges only)"""
        return CommunityGraph(self, n, d, norms_sq, floor)

    def communities_into(self, graph, sset, norms_sq, floor=0.05):
        """mvs_pairwise_community: compare `sset` with itself at level `floor` and feed every kept cell into `graph`, on the device"""
        np_, nm, nk = _norms(norms_sq)
        _check(self.lib.mvs_pairwise_community(self._h, sset._h, np_, nm, float(floor), graph._h))

    def communities(self, sset, norms_sq, floor=0.05, resolution=1.0, max_rounds=100):
        """Modularity communities (Louvain with the connected split) of the graph of Jaccard estimates above `floor` -> Communities.
        All integers: equal to tests/communities_model.py whatever the blocking, the options or the order of the cells."""
        np_, nm, nk = _norms(norms_sq)
        return _communities_call(sset.n, lambda *out: self.lib.mvs_communities(self._h, sset._h, np_, nm, float(floor), float(resolution),
                                                                                int(max_rounds), *out))

    def community_stats(self):
        """-> dict since this context's last CommunityGraph was created: compare_ms, build_ms, move_ms, aggregate_ms, level0_move_ms
        (timing on), edges, levels, rounds, row_blocks, level0_rounds, level0_bytes, paths (vertices that started in the wave /
        workgroup / global path, hand-overs wave -> workgroup and workgroup -> global)"""
        d = [_c.c_double() for _ in range(5)]
        n = [_c.c_int64() for _ in range(6)]
        paths = np.zeros(5, dtype=np.int64)
        _check(self.lib.mvs_ctx_community_stats(self._h, *([ctypes.byref(x) for x in d + n] + [paths.ctypes.data])))
        names = ("compare_ms", "build_ms", "move_ms", "aggregate_ms", "level0_move_ms", "edges", "levels", "rounds", "row_blocks",
                 "level0_rounds", "level0_bytes")
        out = {k: x.value for k, x in zip(names, d + n)}
        out["paths"] = paths.tolist()
        return out

    # ---- t-SNE (include/mvs_hip.h "t-SNE") ----
    def tsne_graph(self, n):
        """-> TsneGraph: an empty graph of affinities and a fresh optimiser state over n samples"""
        return TsneGraph(self, n)

    def tsne(self, sset, norms_sq, perplexity=30, neighbours=None, iterations=750, exaggeration=12, exaggeration_iters=250,
             learning_rate=None, init="pcoa", seed=0):
        """The exact t-SNE map of the Jaccard kNN graph -> Tsne.  Equal to tests/tsne_model.py bit for bit from the same graph and
        initial state, whatever the blocking or the options."""
        if init not in TSNE_INIT:
            raise ValueError("init is 'pcoa' or 'random'")
        p = TsneParams(float(perplexity), float(exaggeration), float(learning_rate or 0.0), int(neighbours or 0), int(iterations),
                       int(exaggeration_iters), TSNE_INIT[init], int(seed))
        np_, nm, nk = _norms(norms_sq)
        n = sset.n
        Y, Y0, beta = np.zeros((n, 2), dtype=np.float64), np.zeros((n, 2), dtype=np.float64), np.zeros(n, dtype=np.float64)
        res, h = TsneResult(), _P()
        _check(self.lib.mvs_tsne(self._h, sset._h, np_, nm, ctypes.byref(p), Y.ctypes.data, Y0.ctypes.data, beta.ctypes.data,
                                 ctypes.byref(res), ctypes.byref(h)))
        with TsneGraph(self, n, _handle=h) as g:
            edges = g.edges()
        return Tsne(res, Y, Y0, beta, edges)

    def tsne_stats(self):
        """-> dict since this context's last TsneGraph was created: topk_ms, calibrate_ms, graph_ms, repulse_ms, attract_ms,
        update_ms (timing on), iterations, entries, units, row_blocks"""
        d = [_c.c_double() for _ in range(6)]
        n = [_c.c_int64() for _ in range(4)]
        _check(self.lib.mvs_ctx_tsne_stats(self._h, *[ctypes.byref(x) for x in d + n]))
        names = ("topk_ms", "calibrate_ms", "graph_ms", "repulse_ms", "attract_ms", "update_ms", "iterations", "entries", "units", "row_blocks")
        return {k: x.value for k, x in zip(names, d + n)}

    def _consumer_stats(self, fn, work_key):
        """what cluster_stats, linkage_stats and derep_stats share: fn is the context's mvs_ctx_*_stats, work_key names the time
        of the consumer's own kernels"""
        a, b = _c.c_double(), _c.c_double()
        e, n, r = _c.c_int64(), _c.c_int64(), _c.c_int64()
        _check(fn(self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(e), ctypes.byref(n), ctypes.byref(r)))
        return {"compare_ms": a.value, work_key: b.value, "edges": e.value, "row_blocks": n.value, "rounds": r.value}

    # ---- single-linkage clustering (include/mvs_hip.h "Single-linkage clustering") ----
    def cluster_into(self, cluster, sset, norms_sq, min_jaccard):
        """mvs_pairwise_cluster: compare `sset` with itself and feed every pair whose Jaccard estimate exceeds min_jaccard
        (0 < min_jaccard < 1) into `cluster`, on the device"""
        np_, nm, nk = _norms(norms_sq)
        _check(self.lib.mvs_pairwise_cluster(self._h, sset._h, np_, nm, float(min_jaccard), cluster._h))

    def cluster(self, sset, norms_sq, min_jaccard):
        """Single-linkage clusters of the samples of `sset` at Jaccard > min_jaccard -> ClusterResult (labels, degree,
        representatives, sizes, n_clusters).  Exact: equal to a brute force over all pairs.  No cell leaves the device."""
        with Cluster(self, sset.n) as k:
            self.cluster_into(k, sset, norms_sq, min_jaccard)
            return k.finish(norms_sq)

    def cluster_stats(self):
        """-> dict since this context's last Cluster was created: compare_ms / union_ms (kernel times, timing on), edges
        (cells with row != col consumed), row_blocks, rounds (most hook -> flatten -> verify rounds a list needed)"""
        return self._consumer_stats(self.lib.mvs_ctx_cluster_stats, "union_ms")

    # ---- the single-linkage tree (include/mvs_hip.h "the single-linkage tree") ----
    def linkage_into(self, linkage, sset, norms_sq, min_jaccard):
        """mvs_pairwise_linkage: compare `sset` with itself and feed every pair whose Jaccard estimate exceeds min_jaccard
        (0 < min_jaccard < 1) into `linkage`, on the device"""
        np_, nm, nk = _norms(norms_sq)
        _check(self.lib.mvs_pairwise_linkage(self._h, sset._h, np_, nm, float(min_jaccard), linkage._h))

    def linkage(self, sset, norms_sq, min_jaccard):
        """The single-linkage tree of the samples of `sset` at Jaccard > min_jaccard -> LinkageResult: the maximum spanning
        forest of the thresholded graph, links sorted best first.  result.cut(u) for any u >= min_jaccard gives the clusters
        Context.cluster(u) would.  Exact: equal to a host Kruskal under the same order.  No cell leaves the device."""
        with Linkage(self, sset.n, sset.d, norms_sq) as k:
            self.linkage_into(k, sset, norms_sq, min_jaccard)
            return k.finish()

    def linkage_stats(self):
        """-> dict since this context's last Linkage was created: compare_ms / forest_ms (kernel times, timing on), edges (fed
        cells with row != col), row_blocks, rounds (most Boruvka rounds a list needed)"""
        return self._consumer_stats(self.lib.mvs_ctx_linkage_stats, "forest_ms")

    # ---- HDBSCAN* (include/mvs_hip.h "HDBSCAN*") ----
    def core_jaccard(self, sset, norms_sq, k, out=None):
        """mvs_core_jaccard: the Jaccard estimate of every sample's k-th nearest neighbour (NaN for a sample with fewer than k
        scored neighbours) -> float64 [n], or `out` (a torch float64 device tensor [n]) filled"""
        np_, nm, nk = _norms(norms_sq)
        if out is None:
            core = np.empty(max(sset.n, 1), dtype=np.float64)
            _check(self.lib.mvs_core_jaccard(self._h, sset._h, np_, nm, int(k), core.ctypes.data, MEM_HOST))
            return core[:sset.n]
        op, om, ok = _buf(out)
        _check(self.lib.mvs_core_jaccard(self._h, sset._h, np_, nm, int(k), op, om))
        return out

    def hdbscan(self, sset, norms_sq, min_samples=5, floor=0.05, min_cluster_size=5, allow_roots=True):
        """mvs_hdbscan: core similarities (k = min_samples), the single-linkage tree of the mutual reachability at Jaccard >
        floor, condensed tree and selection by stability -> Hdbscan with .labels .strength .core .lambda_out .clusters .links.
        No level to choose beyond the floor below which pairs are not compared; no cell leaves the device."""
        n = sset.n
        np_, nm, nk = _norms(norms_sq)
        core, strength = np.empty(max(n, 1), dtype=np.float64), np.zeros(max(n, 1), dtype=np.float64)
        links = np.empty(max(n - 1, 1), dtype=LINK_DTYPE)
        labels, lam = np.full(max(n, 1), -1, dtype=np.int32), np.full(max(n, 1), -1, dtype=np.int64)
        clusters = np.zeros(max(n, 1), dtype=HDBSCAN_CLUSTER_DTYPE)
        n_links, count = _c.c_int64(), _c.c_int64()
        _check(self.lib.mvs_hdbscan(self._h, sset._h, np_, nm, int(min_samples), float(floor), int(min_cluster_size),
                                    0 if allow_roots else HDBSCAN_NO_ROOTS, core.ctypes.data, links.ctypes.data, ctypes.byref(n_links),
                                    labels.ctypes.data, strength.ctypes.data, lam.ctypes.data, clusters.ctypes.data, len(clusters),
                                    ctypes.byref(count)))
        return Hdbscan(labels[:n], strength[:n], lam[:n], clusters[:count.value].copy(), core[:n], LinkageResult(n, links[:n_links.value]))

    def hdbscan_stats(self):
        """-> dict of the last core_jaccard / hdbscan: core_dots_ms, core_select_ms, core_kth_ms, compare_ms, forest_ms (kernel
        times, timing on), host_ms (the selection), ranges (top-k row ranges), rounds, links, edges"""
        t = [_c.c_double() for _ in range(6)]
        v = [_c.c_int64() for _ in range(4)]
        _check(self.lib.mvs_ctx_hdbscan_stats(self._h, *[ctypes.byref(x) for x in t + v]))
        names = ("core_dots_ms", "core_select_ms", "core_kth_ms", "compare_ms", "forest_ms", "host_ms", "ranges", "rounds", "links", "edges")
        return dict(zip(names, (x.value for x in t + v)))

    # ---- greedy dereplication (include/mvs_hip.h "greedy dereplication") ----
    def derep_into(self, derep, sset, norms_sq, min_jaccard):
        """mvs_pairwise_derep: compare `sset` with itself at Jaccard > min_jaccard (0 < min_jaccard < 1) and decide every row
        of `derep` in ROW order, row block by row block, on the device"""
        np_, nm, nk = _norms(norms_sq)
        _check(self.lib.mvs_pairwise_derep(self._h, sset._h, np_, nm, float(min_jaccard), derep._h))

    def dereplicate(self, sset, norms_sq, min_jaccard, order=None):
        """Greedy dereplication of the samples of `sset` at Jaccard > min_jaccard -> DerepResult (rep_of, link_dot, link_q,
        sizes, is_rep, representatives, n_representatives): every member is linked to its representative, no two
        representatives are linked.  order: an int32 permutation, order[0] goes first; None = the largest norms_sq first, equal
        norms by the smaller index, NaN last.  Exact: equal to the sequential walk.  No cell leaves the device."""
        np_, nm, nk = _norms(norms_sq)
        op = None
        if order is not None:
            order = np.ascontiguousarray(order.cpu().numpy() if _is_torch(order) else order, dtype=np.int32)
            if order.shape != (sset.n,):
                raise MvsError(MVS_E_INVALID, "order must have n entries")
            op = order.ctypes.data
        n = sset.n
        rep_of, link_dot = np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int32)
        link_q, sizes = np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int32)
        count = _c.c_int64()
        _check(self.lib.mvs_dereplicate(self._h, sset._h, np_, nm, float(min_jaccard), op, rep_of.ctypes.data,
                                        link_dot.ctypes.data, link_q.ctypes.data, sizes.ctypes.data, MEM_HOST, ctypes.byref(count)))
        res = DerepResult(rep_of, link_dot, link_q, sizes)
        assert res.n_representatives == count.value
        return res

    def derep_stats(self):
        """-> dict since this context's last Derep was created: compare_ms / greedy_ms (kernel times, timing on), edges (cells
        with row != col consumed), row_blocks, rounds (most scan -> decide rounds a row block needed)"""
        return self._consumer_stats(self.lib.mvs_ctx_derep_stats, "greedy_ms")

    # ---- exact hash-set intersections (include/mvs_hip.h "exact hash-set intersections") ----
    def hash_set(self, hashes, offsets):
        """mvs_hash_set_create: hashes = uint64 numpy array or torch tensor (host or device; an int64 view of the bits is
        accepted), offsets = host int64 [n + 1] -> HashSet"""
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        n = len(offsets) - 1
        hp, hm, hk = _buf(hashes) if _is_torch(hashes) else _buf(hashes, np.uint64)
        h = _P()
        _check(self.lib.mvs_hash_set_create(self._h, hp, hm, offsets.ctypes.data, n, ctypes.byref(h)))
        return HashSet(self, h)

    @staticmethod
    def _sample_bytes(seqs):
        """seqs as sketch_sequences / sketch_proteins take them -> (pointer, mem flag, keepalive, offsets int64 [n + 1])"""
        if isinstance(seqs, tuple) and len(seqs) == 2 and not isinstance(seqs[0], (bytes, bytearray, str)):
            bases, offsets = seqs
            offsets = np.ascontiguousarray(offsets, dtype=np.int64)
            if _is_torch(bases):
                if str(bases.dtype) != "torch.uint8":
                    raise ValueError("bases must be uint8")
                bp, bm, bk = _buf(bases)
            else:
                bp, bm, bk = _buf(bases, np.uint8)
        else:
            parts = [x.encode("latin-1") if isinstance(x, str) else bytes(x) for x in seqs]
            offsets = np.zeros(len(parts) + 1, dtype=np.int64)
            if parts:
                np.cumsum([len(x) for x in parts], out=offsets[1:])
            bp, bm, bk = _buf(np.frombuffer(b"".join(parts), dtype=np.uint8), np.uint8)
        if offsets.ndim != 1 or len(offsets) < 1:
            raise ValueError("offsets must hold n + 1 entries")
        return bp, bm, bk, offsets

    # ---- sketches from sequences (include/mvs_hip.h "sketches from sequences") ----
    def sketch_sequences(self, seqs, ksize=31, scaled=1000, seed=42, max_hash=None):
        """mvs_hash_set_from_sequences: the FracMinHash sketches of DNA samples -> HashSet.  seqs: a list of bytes / str, one
        sample each (join the records of a sample with one non-base byte such as b"\\n"), or a pair (bases, offsets) with bases
        a uint8 numpy array or torch tensor (host or device) and offsets host int64 [n + 1].  A value is kept iff it is
        <= max_hash (default: kmer_max_hash(scaled))."""
        bp, bm, bk, offsets = self._sample_bytes(seqs)
        if max_hash is None:
            max_hash = kmer_max_hash(scaled)
        h = _P()
        _check(self.lib.mvs_hash_set_from_sequences(self._h, bp, bm, offsets.ctypes.data, len(offsets) - 1, int(ksize),
                                                     int(seed) & 0xFFFFFFFF, int(max_hash), ctypes.byref(h)))
        return HashSet(self, h)

    # ---- protein sketches (include/mvs_hip.h "protein sketches") ----
    def sketch_proteins(self, seqs, ksize=None, scaled=200, alphabet="protein", translate=False, seed=42, max_hash=None):
        """mvs_hash_set_from_residues: the FracMinHash sketches of protein samples, or with translate=True of DNA samples in all
        six reading frames, in `alphabet` ("protein", "dayhoff", "hp") -> HashSet.  seqs as sketch_sequences takes them.  ksize
        counts residues, 1 .. 64 (default 10 / 16 / 42 by alphabet).  A value is kept iff it is <= max_hash (default:
        kmer_max_hash(scaled))."""
        alpha = _alphabet(alphabet)
        if ksize is None:
            ksize = AA_KSIZE[alphabet]
        bp, bm, bk, offsets = self._sample_bytes(seqs)
        if max_hash is None:
            max_hash = kmer_max_hash(scaled)
        h = _P()
        _check(self.lib.mvs_hash_set_from_residues(self._h, bp, bm, offsets.ctypes.data, len(offsets) - 1,
                                                    SEQ_TRANSLATE if translate else SEQ_PROTEIN, alpha, int(ksize),
                                                    int(seed) & 0xFFFFFFFF, int(max_hash), ctypes.byref(h)))
        return HashSet(self, h)

    def aa_stats(self):
        """-> dict of this context's last sketch_proteins: kernel_ms (timing on), bytes, kmers (hashed k-mers: two per window
        with translate), kept (values <= max_hash before the unique compaction), units of work, second_trips"""
        ms = _c.c_double()
        v = [_c.c_int64() for _ in range(5)]
        _check(self.lib.mvs_ctx_aa_stats(self._h, ctypes.byref(ms), *[ctypes.byref(x) for x in v]))
        return dict(zip(("kernel_ms", "bytes", "kmers", "kept", "units", "second_trips"), [ms.value] + [x.value for x in v]))

    def aa_sample_stats(self, n_samples):
        """-> (kmers, kept): int64 [n_samples] each, per sample of this context's last sketch_proteins"""
        kmers, kept = np.empty(n_samples, dtype=np.int64), np.empty(n_samples, dtype=np.int64)
        _check(self.lib.mvs_ctx_aa_sample_stats(self._h, int(n_samples), kmers.ctypes.data, kept.ctypes.data))
        return kmers, kept

    # ---- abundances (include/mvs_hip.h "abundances") ----
    def kmer_sketcher(self, n_samples, ksize=31, scaled=1000, seed=42, max_hash=None):
        """mvs_kmer_sketcher_create -> KmerSketcher for n_samples read sets"""
        return KmerSketcher(self, n_samples, ksize=ksize, scaled=scaled, seed=seed, max_hash=max_hash)

    def hash_set_counted(self, lists, weights=None, min_abundance=1, max_abundance=0, histogram=False):
        """mvs_hash_set_create_counted: lists = one sequence of 64-bit values per sample (any order, duplicates welcome), or a
        pair (hashes, offsets) as hash_set takes it (hashes ONE flat numpy array or uint64 / int64 tensor, never a list); weights = uint32 aligned with the values (same form as lists), default 1
        each.  -> HashSet with abundances (the sums of the weights of equal values) of the values that pass the filter; with
        histogram=True -> (HashSet, int64 [n, 256])"""
        def flat(x, dtype):
            # (array, offsets): the first entry is ONE flat numpy array / tensor / DeviceArray; anything else is a sequence of samples
            if isinstance(x, tuple) and len(x) == 2 and (_is_torch(x[0]) or isinstance(x[0], (np.ndarray, DeviceArray))):
                if _is_torch(x[0]) and str(x[0].dtype) not in (("torch.uint64", "torch.int64") if dtype == np.uint64 else ("torch.uint32", "torch.int32")):
                    raise ValueError("a tensor of %s is needed (the signed view of the bits is accepted)" % np.dtype(dtype).name)
                return x[0], np.ascontiguousarray(x[1], dtype=np.int64)
            parts = [np.asarray(v, dtype=dtype).reshape(-1) for v in x]
            offsets = np.zeros(len(parts) + 1, dtype=np.int64)
            if parts:
                np.cumsum([len(v) for v in parts], out=offsets[1:])
            return (np.concatenate(parts) if parts else np.empty(0, dtype=dtype)), offsets
        hashes, offsets = flat(lists, np.uint64)
        hp, hm, hk = _buf(hashes) if _is_torch(hashes) else _buf(hashes, np.uint64)
        wp, wm, wk = None, MEM_HOST, None
        if weights is not None:
            w, woff = flat((weights, offsets) if _is_torch(weights) or isinstance(weights, np.ndarray) else weights, np.uint32)
            if woff.tolist() != offsets.tolist():
                raise ValueError("weights must be aligned with the values")
            wp, wm, wk = _buf(w) if _is_torch(w) else _buf(w, np.uint32)
        n = len(offsets) - 1
        hist = np.zeros((n, 256), dtype=np.int64) if histogram else None
        h = _P()
        _check(self.lib.mvs_hash_set_create_counted(self._h, hp, hm, wp, wm, offsets.ctypes.data, n, int(min_abundance), int(max_abundance),
                                                     hist.ctypes.data if histogram else None, ctypes.byref(h)))
        hs = HashSet(self, h)
        return (hs, hist) if histogram else hs

    def abund_stats(self):
        """-> dict of this context's last counted build (KmerSketcher.finish, hash_set_counted): sort_ms, count_ms (kernel times,
        timing on), values_in, distinct, passed, units of the run-sum passes, big_segments (samples sorted device-wide)"""
        t = [_c.c_double(), _c.c_double()]
        v = [_c.c_int64() for _ in range(5)]
        _check(self.lib.mvs_ctx_abund_stats(self._h, *[ctypes.byref(x) for x in t + v]))
        return dict(zip(("sort_ms", "count_ms", "values_in", "distinct", "passed", "units", "big_segments"), (x.value for x in t + v)))

    def kmer_stats(self):
        """-> dict of this context's last sketch_sequences: kernel_ms (timing on), bases, kmers (valid positions), kept (values
        <= max_hash before the unique compaction), units of work, second_trips (hashing passes repeated for a longer list)"""
        ms = _c.c_double()
        v = [_c.c_int64() for _ in range(5)]
        _check(self.lib.mvs_ctx_kmer_stats(self._h, ctypes.byref(ms), *[ctypes.byref(x) for x in v]))
        return dict(zip(("kernel_ms", "bases", "kmers", "kept", "units", "second_trips"), [ms.value] + [x.value for x in v]))

    def kmer_sample_stats(self, n_samples):
        """-> (kmers, kept): int64 [n_samples] each, per sample of this context's last sketch_sequences: valid positions and
        the values <= max_hash before the unique compaction"""
        kmers, kept = np.empty(n_samples, dtype=np.int64), np.empty(n_samples, dtype=np.int64)
        _check(self.lib.mvs_ctx_kmer_sample_stats(self._h, int(n_samples), kmers.ctypes.data, kept.ctypes.data))
        return kmers, kept

    @staticmethod
    def _cells_arg(cells):
        """cells as intersect_cells / abund_overlap take them -> (pointer, mem flag, keepalive, number of cells)"""
        if _is_torch(cells):
            cp, cm, ck = _buf(cells)
            return cp, cm, ck, cells.shape[0]
        a = np.asarray(cells)
        if a.dtype != CELL_DTYPE:
            a = np.asarray(a, dtype=np.int32)
            if a.ndim != 2 or a.shape[1] < 2:
                raise ValueError("cells must be CELL_DTYPE records or an int32 array [m, >= 2]")
            full = np.zeros((a.shape[0], 4), dtype=np.int32)
            full[:, :min(4, a.shape[1])] = a[:, :4]
            a = full
        ck = np.ascontiguousarray(a)
        return ck.ctypes.data, MEM_HOST, ck, ck.shape[0]

    def intersect_cells(self, hs, cells, n_cells=None, hs_cols=None, out=None):
        """inter[i] = |H_rows(cells[i].row) n H_cols(cells[i].col)|, exact (mvs_intersect_cells).  cells: numpy structured
        array (CELL_DTYPE) or int32 [m, 4] / [m, 2+] rows of (row, col, ...), or a torch device tensor int32 [m, 4] (the first
        n_cells rows, default all).  hs_cols: the columns' set (default: hs).  Returns int32 counts: a numpy array for host
        cells, a torch device tensor for device cells, or `out`."""
        cp, cm, ck, m = self._cells_arg(cells)
        if n_cells is None:
            n_cells = m
        elif n_cells > m:
            raise ValueError("n_cells beyond the cell list")
        if out is None:
            if cm == MEM_DEVICE:
                import torch
                out = torch.empty(max(int(n_cells), 0), dtype=torch.int32, device=cells.device)
            else:
                out = np.empty(max(int(n_cells), 0), dtype=np.int32)
        op, om, ok = _buf(out) if _is_torch(out) else _buf(out, np.int32, writable=True)
        _check(self.lib.mvs_intersect_cells(self._h, hs._h, hs_cols._h if hs_cols is not None else None, cp, cm, int(n_cells),
                                            op, om))
        return out

    def exact_jaccard(self, hs, cells, hs_cols=None):
        """-> (inter int32, jaccard, contain_row, contain_col) as numpy arrays, the last three float64 computed above the
        library in this order: J = inter / (|A| + |B| - inter), C_row = inter / |A|, C_col = inter / |B|; 0 / 0 is NaN"""
        inter = self.intersect_cells(hs, cells, hs_cols=hs_cols)
        if _is_torch(inter):
            inter = inter.cpu().numpy()
        if _is_torch(cells):
            rc = cells[:, :2].cpu().numpy()
            rows, cols = rc[:, 0], rc[:, 1]
        else:
            a = np.asarray(cells)
            rows, cols = (a["row"], a["col"]) if a.dtype == CELL_DTYPE else (a[:, 0], a[:, 1])
        sa = hs.sizes()[rows].astype(np.float64)
        sb = (hs_cols if hs_cols is not None else hs).sizes()[cols].astype(np.float64)
        fi = inter.astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            return inter, fi / (sa + sb - fi), fi / sa, fi / sb

    # ---- abundance-weighted overlaps (include/mvs_hip.h "abundance-weighted overlaps") ----
    def abund_overlap(self, hs, cells, n_cells=None, hs_cols=None, out=None):
        """mvs_abund_overlap_cells: per cell inter, w_row, w_col, w_min, dot_lo, dot_hi over the values the two samples share,
        a value of a set without abundances counting 1; exact.  cells and hs_cols as intersect_cells takes them.  Returns
        ABUND_OVERLAP_DTYPE records (numpy) for host cells, a torch device tensor int64 [m, 6] (the bits of the unsigned sums)
        for device cells, or `out`.  Also leaves intersect_stats()."""
        cp, cm, ck, m = self._cells_arg(cells)
        if n_cells is None:
            n_cells = m
        elif n_cells > m:
            raise ValueError("n_cells beyond the cell list")
        if out is None:
            if cm == MEM_DEVICE:
                import torch
                out = torch.empty((max(int(n_cells), 0), 6), dtype=torch.int64, device=cells.device)
            else:
                out = np.empty(max(int(n_cells), 0), dtype=ABUND_OVERLAP_DTYPE)
        if _is_torch(out):
            if str(out.dtype) != "torch.int64" or out.numel() < 6 * int(n_cells):
                raise ValueError("out must be an int64 tensor [n_cells, 6]")
            op, om, ok = _buf(out)
        else:
            if len(out) < int(n_cells):
                raise ValueError("out is shorter than the cell list")
            op, om, ok = _buf(out, ABUND_OVERLAP_DTYPE, writable=True)
        _check(self.lib.mvs_abund_overlap_cells(self._h, hs._h, hs_cols._h if hs_cols is not None else None, cp, cm, int(n_cells),
                                                op, om))
        return out

    def abundance_similarity(self, hs, cells, hs_cols=None):
        """The abundance-weighted measures of every cell -> dict of numpy arrays: inter, w_row, w_col, w_min, dot (object array
        of Python ints: dot_hi * 2^32 + dot_lo), and float64 w_contain_row, w_contain_col, bray_curtis (the dissimilarity),
        ruzicka, cosine, angular -- each computed by mvs_abund_similarity from the record and the samples' totals, so the
        rounding is the library's; 0 / 0 is NaN"""
        rec = self.abund_overlap(hs, cells, hs_cols=hs_cols)
        if _is_torch(rec):
            rec = np.ascontiguousarray(rec.cpu().numpy()).view(ABUND_OVERLAP_DTYPE).reshape(-1)
        if _is_torch(cells):
            rc = cells[:, :2].cpu().numpy()
            rows, cols = rc[:, 0], rc[:, 1]
        else:
            a = np.asarray(cells)
            rows, cols = (a["row"], a["col"]) if a.dtype == CELL_DTYPE else (a[:, 0], a[:, 1])
        cs = hs_cols if hs_cols is not None else hs
        tr, tc = hs.abundance_totals(), (cs.abundance_totals() if cs is not hs else None)
        tc = tr if tc is None else tc
        zr, zc = hs.sizes(), (cs.sizes() if cs is not hs else None)
        zc = zr if zc is None else zc
        derived = np.empty((len(rec), 6), dtype=np.float64)
        for i in range(len(rec)):
            r, c = int(rows[i]), int(cols[i])
            derived[i] = abund_similarity(rec[i], (tr[0][r], tr[1][r], tr[2][r]), zr[r], (tc[0][c], tc[1][c], tc[2][c]), zc[c])
        res = {f: rec[f].copy() for f in ("inter", "w_row", "w_col", "w_min")}
        res["dot"] = np.array([(int(h) << 32) + int(l) for l, h in zip(rec["dot_lo"], rec["dot_hi"])], dtype=object)
        for k, f in enumerate(ABUND_MEASURES):
            res[f] = derived[:, k].copy()
        return res

    def intersect_stats(self):
        """-> dict of this context's last intersect_cells: kernel_ms (timing on), units of work launched, cut_pairs (cells
        that consisted of several units) and bytes = the sum of 8 (|A| + |B|) over its cells"""
        ms, u, k, b = _c.c_double(), _c.c_int64(), _c.c_int64(), _c.c_int64()
        _check(self.lib.mvs_ctx_intersect_stats(self._h, ctypes.byref(ms), ctypes.byref(u), ctypes.byref(k), ctypes.byref(b)))
        return {"kernel_ms": ms.value, "units": u.value, "cut_pairs": k.value, "bytes": b.value}

    # ---- gather (include/mvs_hip.h "gather") ----
    def gather(self, hs_query, query, hs_db, candidates=None, min_hashes=1, max_matches=None):
        """mvs_gather: the greedy decomposition of sample `query` of hs_query into samples of hs_db -- repeatedly the
        candidate with the largest overlap with what is left of the query (ties: the smaller sample index), until the best
        adds fewer than min_hashes hashes or max_matches records exist (None: the number of distinct candidates).
        candidates: sample indices of hs_db (int32 numpy array / sequence, or a torch device tensor; None: every sample;
        order and duplicates do not matter).  -> GatherResult."""
        cp, cm, ck, n_cand = None, MEM_HOST, None, 0
        if candidates is not None:
            if not _is_torch(candidates):
                candidates = np.asarray(candidates, dtype=np.int32).reshape(-1)
            elif str(candidates.dtype) != "torch.int32" or candidates.dim() != 1:
                raise ValueError("candidates must be a one-dimensional int32 tensor")
            n_cand = int(candidates.shape[0])
            if n_cand == 0:                                            # an empty list is not "every sample": a non-NULL pointer
                candidates = np.zeros(1, dtype=np.int32)
            cp, cm, ck = _buf(candidates) if _is_torch(candidates) else _buf(candidates, np.int32)
        if max_matches is None:
            if candidates is None:
                max_matches = hs_db.n
            else:
                max_matches = len(np.unique(ck.cpu().numpy() if _is_torch(ck) else ck)) if n_cand else 0
        out = np.empty(max(int(max_matches), 1), dtype=GATHER_DTYPE)
        count, q_size = _c.c_int64(), _c.c_int32()
        _check(self.lib.mvs_gather(self._h, hs_query._h, int(query), hs_db._h, cp, cm, n_cand, int(min_hashes), int(max_matches),
                                   out.ctypes.data, MEM_HOST, ctypes.byref(count), ctypes.byref(q_size)))
        matches = out[:count.value].copy()
        sizes = hs_db.sizes()[matches["sample"]] if count.value else np.empty(0, dtype=np.int32)
        return GatherResult(matches, q_size.value, sizes)

    def gather_stats(self):
        """-> dict of this context's last gather: survivors (candidates at min_hashes or above before the walk), rounds,
        batches (read-backs of the walk's state), row_bytes (the survivors' bit rows), round_bytes (live rows x row size summed
        over the rounds: what the round passes streamed), overlap_ms / mark_ms / rounds_ms
        (kernel times of the three phases, timing on)"""
        s, r, b, rb = _c.c_int64(), _c.c_int64(), _c.c_int64(), _c.c_int64()
        o, m, t = _c.c_double(), _c.c_double(), _c.c_double()
        _check(self.lib.mvs_ctx_gather_stats(self._h, ctypes.byref(s), ctypes.byref(r), ctypes.byref(b), ctypes.byref(rb),
                                             ctypes.byref(o), ctypes.byref(m), ctypes.byref(t)))
        streamed = _c.c_int64()
        _check(self.lib.mvs_ctx_gather_round_bytes(self._h, ctypes.byref(streamed)))
        return {"survivors": s.value, "rounds": r.value, "batches": b.value, "row_bytes": rb.value, "overlap_ms": o.value,
                "mark_ms": m.value, "rounds_ms": t.value, "round_bytes": streamed.value}

    def pairwise_dots(self, sset, r0, r1, c0, c1, algo=0, out=None):
        if out is None:
            out = np.empty((r1 - r0, c1 - c0), dtype=np.int32)
        op, om, ok = _buf(out, np.int32, writable=True)
        _check(self.lib.mvs_pairwise_dots(self._h, sset._h, r0, r1, c0, c1, op, om, algo))
        return out


def chunk_size(max_memory_gb, d):
    return load_library().mvs_chunk_size(float(max_memory_gb), int(d))


def shard_layout(n_total, world):
    """(rows per shard = ceil(n / world), the same rounded up to a multiple of 256: the block size in storage coordinates)"""
    a, b = _c.c_int64(), _c.c_int64()
    _check(load_library().mvs_shard_layout(int(n_total), int(world), ctypes.byref(a), ctypes.byref(b)))
    return a.value, b.value


PROJ_UNIT_DTYPE = np.dtype([("begin", "<i8"), ("count", "<i4"), ("sample", "<i4"), ("single", "<i4"), ("flags", "<i4")])


def project_plan(offsets, ny, slots, balance=True, overhead=-1):
    """mvs_project_plan: the projection's units of work for the samples of `offsets` (structured array, PROJ_UNIT_DTYPE)"""
    off = np.ascontiguousarray(offsets, dtype=np.int64)
    lib, n = load_library(), _c.c_int64()
    args = (off.ctypes.data, len(off) - 1, int(ny), int(slots), int(overhead), int(bool(balance)))
    _check(lib.mvs_project_plan(*args, None, 0, ctypes.byref(n)))
    units = np.empty(n.value, dtype=PROJ_UNIT_DTYPE)
    _check(lib.mvs_project_plan(*args, units.ctypes.data, len(units), ctypes.byref(n)))
    return units


def shard_rows(n, num_shards, shard_idx):
    b, e = _c.c_int64(), _c.c_int64()
    load_library().mvs_shard_rows(n, num_shards, shard_idx, ctypes.byref(b), ctypes.byref(e))
    return b.value, e.value


def limbs_for_max_abs(max_abs):
    return load_library().mvs_limbs_for_max_abs(int(max_abs))
