"""ctypes binding of libpecanpy_amd.so (the C ABI declared in include/pecanpy_amd.h).

There is no CPU fallback: if the shared library is missing or no GPU is visible the walk operator
raises, loudly.  ``build()`` compiles the library in-tree with hipcc (cross-compiles without a GPU).
"""
import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PECANPY_AMD_LIB") or os.path.join(_HERE, "libpecanpy_amd.so")  # env override: A/B kernel variants
_lib = None


class PwStats(C.Structure):
    _fields_ = [
        ("total_steps", C.c_uint64),
        ("overflow_reads", C.c_uint64),
        ("clamped_reads", C.c_uint64),
        ("dead_end_walks", C.c_uint64),
        ("repair_rounds", C.c_uint64),
        ("walk_kernel_ms", C.c_double),
        ("rng_kernel_ms", C.c_double),
        ("walk_kernel_launches", C.c_uint32),
        ("stream_addressing", C.c_uint32),
        ("lane_kernel", C.c_uint32),
        ("lane_rounds", C.c_uint32),
        ("redo_walks", C.c_uint64),
        ("list_entries_read", C.c_uint64),
        ("ambiguous_steps", C.c_uint64),
        ("lane_kernel_ms", C.c_double),
        ("wave_chain_steps", C.c_uint64),
        ("param_index_ms", C.c_double),
        ("verify_checked", C.c_uint64),
        ("verify_mismatch", C.c_uint64),
        ("verify_dropped", C.c_uint64),
        ("verify_ties", C.c_uint64),
        ("eager_steps", C.c_uint64),
        ("index_max_list", C.c_uint32),
        ("reserved0", C.c_uint32),
    ]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class PwSgnsStats(C.Structure):
    """``pw_sgns_stats`` of include/pecanpy_amd.h."""
    _fields_ = [
        ("vocab_ms", C.c_double),
        ("init_ms", C.c_double),
        ("train_ms", C.c_double),
        ("kept_occurrences", C.c_uint64),
        ("trained_pairs", C.c_uint64),
        ("wavefronts", C.c_uint64),
    ]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class PwSgnsEpoch(C.Structure):
    """``pw_sgns_epoch`` of include/pecanpy_amd.h."""
    _fields_ = [
        ("loss", C.c_double),
        ("kept_occurrences", C.c_uint64),
        ("trained_pairs", C.c_uint64),
        ("evaluations", C.c_uint64),
    ]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class PwSgnsState(C.Structure):
    """``pw_sgns_state`` of include/pecanpy_amd.h."""
    _fields_ = [
        ("epoch", C.c_uint64),
        ("sched_pos", C.c_uint64),
        ("sched_total", C.c_uint64),
        ("alpha", C.c_float),
        ("min_alpha", C.c_float),
    ]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


PW_SGNS_LOSS = 1
PW_SGNS_RECOUNT = 1   # pw_sgns_set_walks


class PwEmbWriteStats(C.Structure):
    """``pw_emb_write_stats`` of include/pecanpy_amd.h."""
    _fields_ = [
        ("format_ms", C.c_double),
        ("copy_ms", C.c_double),
        ("write_ms", C.c_double),
        ("bytes", C.c_uint64),
        ("chunks", C.c_uint64),
    ]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class PwWalksWriteStats(C.Structure):
    """``pw_walks_write_stats`` of include/pecanpy_amd.h."""
    _fields_ = [
        ("format_ms", C.c_double),
        ("copy_ms", C.c_double),
        ("write_ms", C.c_double),
        ("bytes", C.c_uint64),
        ("chunks", C.c_uint64),
        ("rows", C.c_uint64),
        ("tokens", C.c_uint64),
    ]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class PwKnnStats(C.Structure):
    """``pw_knn_stats`` of include/pecanpy_amd.h."""
    _fields_ = [
        ("score_ms", C.c_double),
        ("merge_ms", C.c_double),
        ("total_ms", C.c_double),
        ("grid", C.c_uint32),
        ("row_parts", C.c_uint32),
        ("rows_per_block", C.c_uint32),
        ("queries_per_tile", C.c_uint32),
        ("col_chunk", C.c_uint32),
        ("batches", C.c_uint32),
    ]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class PwKnnTiles(C.Structure):
    """``pw_knn_tiles`` of include/pecanpy_amd.h (0 in a field = the default)."""
    _fields_ = [
        ("rows_per_block", C.c_uint32),
        ("queries_per_tile", C.c_uint32),
        ("grid", C.c_uint32),
        ("col_chunk", C.c_uint32),
    ]


PW_KNN_MAX_TOPN = 128
KNN_METRICS = {"dot": 0, "cosine": 1}   # PW_KNN_DOT, PW_KNN_COSINE
KNN_QT = 8                              # queries a wavefront keeps accumulators for (csrc/knn.hip.h)
NBR_KINDS = {"common_neighbours": 0, "jaccard": 1, "preferential_attachment": 2, "weighted": 3}   # PW_NBR_* (csrc/nbr_scores.hip.h)
LOGIT_OPS = {"row": 0, "average": 1, "hadamard": 2, "l1": 3, "l2": 4}   # PW_LOGIT_* (csrc/logit.hip.h)
LOGIT_MAX_DIM = 512                     # the trainer's cap (LG_MAX_DIM)
LOGIT_CHUNK = 1024                      # LG_CHUNK: part of the definition
NBR_ALL_LANE = 0xFFFFFFFF               # short_max of pw_selftest_nbr_scores: every pair stays with its lane; -1: the default
ERR_INVALID = -1                        # PW_ERR_INVALID


class PwEdgelistDevStats(C.Structure):
    """``pw_edgelist_dev_stats`` of include/pecanpy_amd.h."""
    _fields_ = [
        ("upload_ms", C.c_double),
        ("scan_ms", C.c_double),
        ("ids_ms", C.c_double),
        ("build_ms", C.c_double),
        ("lines", C.c_uint64),
        ("n_nodes", C.c_uint64),
        ("file_bytes", C.c_uint64),
    ]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class PwCorpusDevStats(C.Structure):
    """``pw_corpus_dev_stats`` of include/pecanpy_amd.h."""
    _fields_ = [
        ("upload_ms", C.c_double),
        ("scan_ms", C.c_double),
        ("tokens_ms", C.c_double),
        ("fill_ms", C.c_double),
        ("file_bytes", C.c_uint64),
        ("lines", C.c_uint64),
        ("tokens", C.c_uint64),
        ("names", C.c_uint64),
    ]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class PwSeqConfig(C.Structure):
    """``pw_seq_config`` of include/pecanpy_amd.h (0 in a field = the default)."""
    _fields_ = [
        ("jobs_per_round", C.c_uint32),
        ("max_candidates", C.c_uint32),
        ("word_buffer_blocks", C.c_uint32),
        ("min_jobs", C.c_uint64),
        ("window_sigmas", C.c_float),
        ("force_mean", C.c_float),
        ("force_sigma", C.c_float),
    ]


class PwSeqInfo(C.Structure):
    """``pw_seq_info`` of include/pecanpy_amd.h."""
    _fields_ = [
        ("path", C.c_uint32),
        ("rounds", C.c_uint64),
        ("candidate_walks", C.c_uint64),
        ("committed_jobs", C.c_uint64),
        ("window_misses", C.c_uint64),
        ("unfinished_retries", C.c_uint64),
        ("words_consumed", C.c_uint64),
        ("words_expanded", C.c_uint64),
        ("plan_ms", C.c_double),
        ("candidate_ms", C.c_double),
        ("resolve_ms", C.c_double),
        ("commit_ms", C.c_double),
        ("expand_ms", C.c_double),
    ]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


SEQ_ALWAYS_SEQUENTIAL = 2**64 - 1   # pw_seq_config.min_jobs: the plain sequential loop

EDGELIST_OK, EDGELIST_NEEDS_HOST_READER, EDGELIST_IO = 0, 1, 2   # pw_edgelist_read_device's non-negative results (pw_corpus_read_device's too)
EDGELIST_KEEP_F64 = 1   # pw_edgelist_read_device_ex's flag bit: the CSR keeps the float64 weights for the dense build
ERR_UNSUPPORTED = -4    # PW_ERR_UNSUPPORTED

MODE_IDS = {
    "SparseOTF": 0,
    "DenseOTF": 1,
    "PreComp": 2,
    "FirstOrderUnweighted": 3,
    "PreCompFirstOrder": 4,
    "Node2vecPlusPlus": 5,   # experimental.Node2vecPlusPlus (dense handles)
    "SparseNode2vecPlusPlus": 6,   # experimental.SparseNode2vecPlusPlus (CSR handles)
}

# every symbol include/pecanpy_amd.h declares: (restype, argtypes)
_u32p = C.POINTER(C.c_uint32)
_f32p = C.POINTER(C.c_float)
_f64p = C.POINTER(C.c_double)
_SIM_ARGS = [C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_int, C.c_void_p, C.c_uint64, C.c_uint32,
             C.c_int, C.c_uint32, C.c_uint64, C.c_void_p, C.POINTER(PwStats)]
SYMBOLS = {
    "pw_version": (C.c_char_p, []),
    "pw_last_error": (C.c_char_p, []),
    "pw_device_count": (C.c_int, []),
    "pw_warmup": (C.c_int, [C.c_int, _f64p]),
    "pw_csr_create": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_int,
                                C.POINTER(C.c_void_p)]),
    "pw_coo_to_csr_device": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_int,
                                       C.POINTER(C.c_void_p)]),
    "pw_csr_dev_shape": (C.c_int, [C.c_void_p] + [C.POINTER(C.c_uint64)] * 4 + [C.POINTER(C.c_double)]),
    "pw_csr_dev_export": (C.c_int, [C.c_void_p] * 4),
    "pw_csr_dev_destroy": (None, [C.c_void_p]),
    "pw_csr_create_device": (C.c_int, [C.c_void_p] * 4 + [C.POINTER(C.c_void_p)]),
    "pw_graph_index_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "pw_lane_index_export": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pw_dense_create": (C.c_int, [C.c_void_p, C.c_uint32, C.c_int, C.POINTER(C.c_void_p)]),
    "pw_dense_create_bits": (C.c_int, [C.c_void_p, C.c_uint32, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "pw_dense_create_device": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_uint32, C.POINTER(C.c_void_p), C.POINTER(C.c_double)]),
    "pw_dense_create_from_csr": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_double)]),
    "pw_dense_noise_thresholds": (C.c_int, [C.c_void_p, C.c_double, C.c_void_p]),
    "pw_dense_shape": (C.c_int, [C.c_void_p, _u32p, _u32p, _u32p, _u32p]),
    "pw_dense_export": (C.c_int, [C.c_void_p] * 6 + [_u32p]),
    "pw_graph_set_thresholds": (C.c_int, [C.c_void_p, C.c_void_p]),
    "pw_graph_destroy": (None, [C.c_void_p]),
    "pw_simulate": (C.c_int, _SIM_ARGS),
    "pw_simulate_device": (C.c_int, _SIM_ARGS),
    "pw_graph_replicate": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]),
    "pw_device_mask_to_list": (C.c_int, [C.c_uint64, C.POINTER(C.c_int), C.c_int]),
    "pw_csr_create_multi": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_int), C.c_int,
                                      C.POINTER(C.c_void_p)]),
    "pw_simulate_multi": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, C.c_void_p, C.c_uint64,
                                    C.c_uint32, C.c_int, C.c_uint32, C.c_uint64, C.c_void_p, C.c_int, C.POINTER(PwStats)]),
    "pw_step": (C.c_int, [C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_int, C.c_uint32, C.c_int, C.c_uint32, C.c_double,
                          _u32p, _u32p]),
    "pw_probs": (C.c_int, [C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_int, C.c_uint32, C.c_int, C.c_uint32, C.c_void_p,
                           _u32p]),
    "pw_precomp_build": (C.c_int, [C.c_void_p, C.c_double, C.c_double, C.c_int, C.c_int]),
    "pw_precomp_export": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]),
    "pw_count_stream_draws": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32,
                                        C.POINTER(C.c_uint64)]),
    "pw_stream_hold": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint64]),
    "pw_stream_release": (C.c_int, [C.c_void_p]),
    "pw_sgns_train": (C.c_int, [C.c_int, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                C.c_uint32, C.c_float, C.c_float, C.c_float, C.c_uint32, C.c_uint32, C.c_void_p]),
    "pw_sgns_train_device": (C.c_int, [C.c_int, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                       C.c_uint32, C.c_float, C.c_float, C.c_float, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]),
    "pw_sgns_create_device": (C.c_int, [C.c_int, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                        C.c_uint32, C.c_float, C.c_float, C.c_float, C.c_uint32, C.c_uint32, C.c_uint32,
                                        C.POINTER(C.c_void_p)]),
    "pw_sgns_run": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]),
    "pw_sgns_get_state": (C.c_int, [C.c_void_p, C.POINTER(PwSgnsState)]),
    "pw_sgns_set_state": (C.c_int, [C.c_void_p, C.POINTER(PwSgnsState)]),
    "pw_sgns_vectors_get": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "pw_sgns_vectors_set": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "pw_sgns_evaluate": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint64, C.POINTER(PwSgnsEpoch)]),
    "pw_sgns_set_walks": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32]),
    "pw_sgns_set_locks": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "pw_sgns_get_locks": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "pw_sgns_lock_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "pw_sgns_destroy": (None, [C.c_void_p]),
    "pw_vectors_write_text_device": (C.c_int, [C.c_int, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_char_p,
                                               C.POINTER(PwEmbWriteStats)]),
    "pw_vectors_write_text": (C.c_int, [C.c_int, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_char_p,
                                        C.POINTER(PwEmbWriteStats)]),
    "pw_walks_write_text_device": (C.c_int, [C.c_int, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64, C.c_char_p,
                                             C.POINTER(PwWalksWriteStats)]),
    "pw_walks_write_text": (C.c_int, [C.c_int, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64, C.c_char_p,
                                      C.POINTER(PwWalksWriteStats)]),
    "pw_knn_create_device": (C.c_int, [C.c_int, C.c_void_p, C.c_uint64, C.c_uint32, C.POINTER(C.c_void_p)]),
    "pw_knn_create": (C.c_int, [C.c_int, C.c_void_p, C.c_uint64, C.c_uint32, C.POINTER(C.c_void_p)]),
    "pw_knn_query_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                      C.POINTER(PwKnnStats)]),
    "pw_knn_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), _u32p, C.POINTER(C.c_uint64)]),
    "pw_knn_norms_get": (C.c_int, [C.c_void_p, C.c_void_p]),
    "pw_knn_destroy": (None, [C.c_void_p]),
    "pw_selftest_knn": (C.c_int, [C.c_int, C.c_int, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32,
                                  C.c_int, C.c_int, C.POINTER(PwKnnTiles), C.c_void_p, C.c_void_p]),
    "pw_knn_score_pairs_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p]),
    "pw_auc_device": (C.c_int, [C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]),
    "pw_sample_non_edges_device": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]),
    "pw_selftest_score_pairs": (C.c_int, [C.c_int, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p,
                                          C.c_void_p, C.c_uint64, C.c_int, C.c_void_p]),
    "pw_selftest_auc": (C.c_int, [C.c_int, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]),
    "pw_selftest_sample_non_edges": (C.c_int, [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64,
                                               C.c_uint64, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]),
    "pw_nbr_degrees_device": (C.c_int, [C.c_void_p, C.c_void_p]),
    "pw_nbr_scores_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_void_p]),
    "pw_nbr_scores_device_cut": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_void_p, C.c_int64,
                                           C.POINTER(C.c_float)]),
    "pw_selftest_nbr_scores": (C.c_int, [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int,
                                         C.c_void_p, C.c_int64, C.c_void_p]),
    "pw_selftest_nbr_degrees": (C.c_int, [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]),
    "pw_logit_eval_device": (C.c_int, [C.c_void_p] * 5 + [C.c_uint64, C.c_int, C.c_void_p, C.c_double, _f64p, C.c_void_p, C.c_void_p]),
    "pw_logit_eval_device_grid": (C.c_int, [C.c_void_p] * 5 + [C.c_uint64, C.c_int, C.c_void_p, C.c_double, _f64p, C.c_void_p, C.c_void_p, C.c_int,
                                            C.POINTER(C.c_float)]),
    "pw_selftest_logit": (C.c_int, [C.c_int, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_uint64, C.c_int, C.c_void_p, C.c_double, C.c_int, _f64p, C.c_void_p, C.c_void_p]),
    "pw_selftest_logit_math": (C.c_int, [C.c_int, C.c_void_p, C.c_uint64, C.c_void_p]),
    "pw_holdout_edges_device": (C.c_int, [C.c_void_p, C.c_int, C.c_uint32, C.c_uint64, C.c_uint32, C.c_int, C.POINTER(C.c_void_p),
                                          C.POINTER(C.c_void_p), _f64p]),
    "pw_holdout_dev_shape": (C.c_int, [C.c_void_p] + [C.POINTER(C.c_uint64)] * 3),
    "pw_holdout_dev_fill": (C.c_int, [C.c_void_p] * 4),
    "pw_holdout_dev_destroy": (None, [C.c_void_p]),
    "pw_selftest_holdout_edges": (C.c_int, [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_uint32, C.c_uint64,
                                            C.c_uint32, C.c_int, C.c_uint64] + [C.c_void_p] * 6 + [C.POINTER(C.c_uint64)]),
    "pw_selftest_format_f6":(C.c_int, [C.c_int, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]),
    "pw_selftest_exclusive_scan": (C.c_int, [C.c_int, C.c_int, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]),
    "pw_mt_random_sample": (C.c_int, [C.c_uint32, C.c_uint64, C.c_uint64, C.c_void_p]),
    "pw_stream_sample_device": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint64, C.c_void_p]),
    "pw_mt_words": (C.c_int, [C.c_uint32, C.c_uint64, C.c_uint64, C.c_void_p]),
    "pw_stream_words_device": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint64, C.c_void_p]),
    "pw_selftest_seq_offsets": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32,
                                          C.POINTER(PwSeqConfig), C.c_void_p, C.POINTER(PwSeqInfo)]),
    "pw_selftest_seq_walks": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(PwSeqConfig), C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.POINTER(PwSeqInfo)]),
    "pw_noise_thresholds_csr": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_double, C.c_void_p]),
    "pw_noise_thresholds_csr_numpy1": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_double, C.c_void_p]),
    "pw_selftest_thresholds_row": (C.c_int, [C.c_void_p, C.c_uint64, C.c_double, C.c_void_p]),
    "pw_noise_thresholds_dense": (C.c_int, [C.c_void_p, C.c_uint32, C.c_double, C.c_void_p]),
    "pw_noise_thresholds_csr_f64": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_double, C.c_void_p]),
    "pw_edgelist_read": (C.c_int, [C.c_char_p, C.c_int, C.c_int, C.c_char_p, C.POINTER(C.c_void_p)]),
    "pw_edgelist_shape": (C.c_int, [C.c_void_p] + [C.POINTER(C.c_uint64)] * 4),
    "pw_edgelist_export": (C.c_int, [C.c_void_p] * 7),
    "pw_edgelist_destroy": (None, [C.c_void_p]),
    "pw_edgelist_read_device": (C.c_int, [C.c_char_p, C.c_int, C.c_int, C.c_char_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                          C.POINTER(PwEdgelistDevStats)]),
    "pw_edgelist_read_device_ex": (C.c_int, [C.c_char_p, C.c_int, C.c_int, C.c_char_p, C.c_int, C.c_uint32, C.POINTER(C.c_void_p),
                                             C.POINTER(C.c_void_p), C.POINTER(PwEdgelistDevStats)]),
    "pw_csr_dev_export_f64": (C.c_int, [C.c_void_p, C.c_void_p]),
    "pw_edgelist_ids_shape": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "pw_edgelist_ids_export": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "pw_edgelist_ids_destroy": (None, [C.c_void_p]),
    "pw_corpus_read_device": (C.c_int, [C.c_char_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(PwCorpusDevStats)]),
    "pw_corpus_dev_shape": (C.c_int, [C.c_void_p] + [C.POINTER(C.c_uint64)] * 3),
    "pw_corpus_dev_fill": (C.c_int, [C.c_void_p, C.c_void_p]),
    "pw_corpus_dev_export": (C.c_int, [C.c_void_p, C.c_void_p]),
    "pw_corpus_dev_destroy": (None, [C.c_void_p]),
    "pw_selftest_edgelist_weight": (C.c_int, [C.c_char_p, C.c_uint64, _f64p]),
    "pw_selftest_edgelist_line": (C.c_int, [C.c_char_p, C.c_uint64, C.c_uint64, C.c_char_p, C.c_int, _u32p, C.c_void_p, _f64p]),
    "pw_selftest_exact_decision": (C.c_int, [C.c_void_p, C.c_uint32, C.c_float, C.c_float, C.c_void_p, C.c_uint32,
                                             C.c_void_p, C.c_void_p]),
    "pw_selftest_lane": (C.c_int, [C.c_int, C.c_int, C.c_void_p, C.c_uint32, C.c_float, C.c_float, C.c_void_p, C.c_uint32,
                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pw_selftest_lane_floats": (C.c_int, [C.c_int, C.c_int, C.c_void_p, C.c_uint32, C.c_float, C.c_float, C.c_void_p, C.c_uint32,
                                          C.c_void_p, C.c_void_p, C.c_void_p]),
    "pw_selftest_lane_unit_bounded": (C.c_int, [C.c_void_p, C.c_uint32, C.c_float, C.c_float, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]),
    "pw_selftest_lane_unit_tight": (C.c_int, [C.c_void_p, C.c_uint32, C.c_float, C.c_float, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pw_selftest_lane_weighted": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]),
    "pw_selftest_exact_decision_f64": (C.c_int, [C.c_void_p, C.c_uint32, C.c_double, C.c_double, C.c_void_p,
                                                 C.c_uint32, C.c_void_p, C.c_void_p]),
    "pw_selftest_seqscan_f32": (C.c_int, [C.c_void_p, C.c_uint32, C.c_double, C.c_int, C.c_uint32,
                                          _u32p, _f32p]),
    "pw_selftest_seqscan_f64": (C.c_int, [C.c_void_p, C.c_uint32, C.c_double, C.c_int, C.c_uint32,
                                          _u32p, _f64p]),
}


class PwError(RuntimeError):
    pass


def build(verbose=False):
    """Compile libpecanpy_amd.so for gfx950 with hipcc (in-tree, so it travels with the repo)."""
    cmd = ["make", "-C", os.path.join(_HERE, "csrc")]
    res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if verbose or res.returncode != 0:
        print(res.stdout)
    if res.returncode != 0:
        raise PwError("building libpecanpy_amd.so failed:\n" + res.stdout)
    return LIB_PATH


def load():
    """Load the shared library and type every exported symbol."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise PwError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C pecanpy_amd/csrc` -- the walk engine has no CPU fallback."
        )
    try:  # share torch's HIP runtime (same soname) when torch is used for device buffers / RCCL
        import torch  # noqa: F401
    except Exception:  # pragma: no cover
        pass
    lib = C.CDLL(LIB_PATH)
    for name, (restype, argtypes) in SYMBOLS.items():
        fn = getattr(lib, name)  # AttributeError if the library lacks a declared symbol
        fn.restype = restype
        fn.argtypes = argtypes
    _lib = lib
    return lib


_warm = {"thread": None, "ms": None}


def warmup_async(device=0):
    """Start the library's one-time start-up on `device` (pw_warmup: ~140 ms for the first stream a process creates through the
    library) on a helper thread and return at once: callers with host work in front of their first graph handle -- reading an edge
    list, generating a graph -- call this first and find the runtime warm.  Harmless without a GPU or without the library (nothing
    happens); `warmup_ms()` tells what it took once it is done."""
    import threading

    if _warm["thread"] is not None or not os.path.exists(LIB_PATH):
        return

    def run():
        try:
            ms = C.c_double(0.0)
            if load().pw_warmup(C.c_int(device), C.byref(ms)) == 0:
                _warm["ms"] = ms.value
        except Exception:  # noqa: BLE001 (a warm-up that cannot run changes nothing: the first handle pays the start-up)
            pass

    _warm["thread"] = threading.Thread(target=run, name="pecanpy_amd-warmup", daemon=True)
    _warm["thread"].start()
    import atexit

    atexit.register(lambda: _warm["thread"].join(timeout=5.0))   # (the interpreter does not leave while the runtime is starting)


def warmup_ms():
    """Wall clock of the finished warm-up in ms, or None (not started / still running / no GPU)."""
    t = _warm["thread"]
    if t is not None and not t.is_alive():
        return _warm["ms"]
    return None


def check(rc):
    if rc != 0:
        msg = load().pw_last_error()
        raise PwError(f"libpecanpy_amd error {rc}: {msg.decode() if msg else '?'}")
