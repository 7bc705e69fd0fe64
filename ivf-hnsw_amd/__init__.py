"""ctypes binding of libivfhnsw_hip.so (include/ivfhnsw_hip.h) for the tests and bench.py.

The product is the shared library; this module adds nothing but argument marshalling.  There is no
fallback of any kind: if the library is missing or no gfx950 device is present, calls raise.

The directory name has a hyphen (it mirrors the reference's name), so it is loaded through
`__graft_entry__.load_pkg()` rather than a plain import.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("IVFHNSW_HIP_LIB") or os.path.join(_HERE, "libivfhnsw_hip.so")  # override: A/B runs of two builds

OK, ERR_INVALID, ERR_HIP, ERR_STATE, ERR_NOMEM = 0, -1, -2, -3, -4
FILTER_ALLOW, FILTER_DENY = 0, 1
FILTER_SLOTS, SLOT_NONE = 32, 0xff
TAG_NONE = 0xffff
VALUE_NONE = 0xffffffff
RECON_ORIGINAL, RECON_ROTATED = 0, 1
STAGES = ("opq", "coarse", "lut", "plan", "scan", "select")

# every symbol include/ivfhnsw_hip.h declares
ABI_SYMBOLS = (
    "ivfhnsw_gpu_last_error", "ivfhnsw_gpu_abi_version", "ivfhnsw_gpu_create", "ivfhnsw_gpu_create_view", "ivfhnsw_gpu_destroy",
    "ivfhnsw_gpu_set_stream", "ivfhnsw_gpu_sync", "ivfhnsw_gpu_upload_ivf", "ivfhnsw_gpu_upload_ivf_synthetic",
    "ivfhnsw_gpu_upload_grouping", "ivfhnsw_gpu_upload_quantizer", "ivfhnsw_gpu_search", "ivfhnsw_gpu_search_dev",
    "ivfhnsw_gpu_resolve_keys_dev", "ivfhnsw_gpu_coarse_dev", "ivfhnsw_gpu_coarse", "ivfhnsw_gpu_set_profiling",
    "ivfhnsw_gpu_get_stage_ms", "ivfhnsw_gpu_reset_stage_ms", "ivfhnsw_gpu_last_scan_counts",
    "ivfhnsw_gpu_memory_bytes", "ivfhnsw_gpu_upload_codebooks", "ivfhnsw_gpu_encode",
    "ivfhnsw_gpu_encode_groups", "ivfhnsw_gpu_rotate_dev", "ivfhnsw_gpu_last_scan_kernel",
    "ivfhnsw_gpu_last_stream_dev", "ivfhnsw_gpu_replay_stream_dev", "ivfhnsw_gpu_pq_train", "ivfhnsw_gpu_xty",
    "ivfhnsw_gpu_prepare_latency", "ivfhnsw_gpu_set_batch_split", "ivfhnsw_gpu_last_batch_parts", "ivfhnsw_gpu_search_keys", "ivfhnsw_gpu_resolve_keys", "ivfhnsw_gpu_last_stream",
    "ivfhnsw_gpu_device_count", "ivfhnsw_gpu_knn", "ivfhnsw_gpu_knn_dev", "ivfhnsw_gpu_build_graph", "ivfhnsw_gpu_set_option", "ivfhnsw_gpu_search_sharded",
    "ivfhnsw_gpu_upload_base", "ivfhnsw_gpu_upload_base_dev", "ivfhnsw_gpu_rerank_dev", "ivfhnsw_gpu_rerank",
    "ivfhnsw_gpu_kmeans", "ivfhnsw_gpu_kmeans_dev", "ivfhnsw_gpu_append_ivf", "ivfhnsw_gpu_append_ivf_dev",
    "ivfhnsw_gpu_add", "ivfhnsw_gpu_add_dev", "ivfhnsw_gpu_download_ivf", "ivfhnsw_gpu_remove_ids",
    "ivfhnsw_gpu_remove_ids_dev", "ivfhnsw_gpu_download_grouping", "ivfhnsw_gpu_append_grouping",
    "ivfhnsw_gpu_append_grouping_dev", "ivfhnsw_gpu_add_groups", "ivfhnsw_gpu_add_groups_dev",
    "ivfhnsw_gpu_download_grouping_tables", "ivfhnsw_gpu_upload_centroid_norms",
    "ivfhnsw_gpu_exact_search", "ivfhnsw_gpu_exact_search_dev",
    "ivfhnsw_gpu_build_graph_dev", "ivfhnsw_gpu_last_graph_longest_reverse",
    "ivfhnsw_gpu_set_filter", "ivfhnsw_gpu_set_filter_dev", "ivfhnsw_gpu_clear_filter", "ivfhnsw_gpu_filter_info",
    "ivfhnsw_gpu_range_search", "ivfhnsw_gpu_range_search_dev", "ivfhnsw_gpu_range_results", "ivfhnsw_gpu_range_results_dev",
    "ivfhnsw_gpu_locate", "ivfhnsw_gpu_locate_dev", "ivfhnsw_gpu_reconstruct_rows", "ivfhnsw_gpu_reconstruct_rows_dev",
    "ivfhnsw_gpu_reconstruct", "ivfhnsw_gpu_reconstruct_dev", "ivfhnsw_gpu_search_reconstruct",
    "ivfhnsw_gpu_search_reconstruct_dev",
    "ivfhnsw_gpu_exact_range_search", "ivfhnsw_gpu_exact_range_search_dev", "ivfhnsw_gpu_exact_range_results",
    "ivfhnsw_gpu_exact_range_results_dev",
    "ivfhnsw_gpu_set_base_filter", "ivfhnsw_gpu_set_base_filter_dev", "ivfhnsw_gpu_clear_base_filter",
    "ivfhnsw_gpu_base_filter_info",
    "ivfhnsw_gpu_set_base_filter_slot", "ivfhnsw_gpu_set_base_filter_slot_dev", "ivfhnsw_gpu_clear_base_filter_slot",
    "ivfhnsw_gpu_base_filter_slot_info",
    "ivfhnsw_gpu_exact_search_slots", "ivfhnsw_gpu_exact_search_slots_dev",
    "ivfhnsw_gpu_exact_range_search_slots", "ivfhnsw_gpu_exact_range_search_slots_dev",
    "ivfhnsw_gpu_set_filter_slot", "ivfhnsw_gpu_set_filter_slot_dev", "ivfhnsw_gpu_clear_filter_slot",
    "ivfhnsw_gpu_filter_slot_info", "ivfhnsw_gpu_search_slots", "ivfhnsw_gpu_search_slots_dev",
    "ivfhnsw_gpu_range_search_slots", "ivfhnsw_gpu_range_search_slots_dev",
    "ivfhnsw_gpu_set_tags", "ivfhnsw_gpu_set_tags_dev", "ivfhnsw_gpu_clear_tags", "ivfhnsw_gpu_tags_info",
    "ivfhnsw_gpu_tag_rows", "ivfhnsw_gpu_search_tags", "ivfhnsw_gpu_search_tags_dev",
    "ivfhnsw_gpu_range_search_tags", "ivfhnsw_gpu_range_search_tags_dev",
    "ivfhnsw_gpu_set_values", "ivfhnsw_gpu_set_values_dev", "ivfhnsw_gpu_clear_values", "ivfhnsw_gpu_values_info",
    "ivfhnsw_gpu_value_rows", "ivfhnsw_gpu_search_values", "ivfhnsw_gpu_search_values_dev",
    "ivfhnsw_gpu_range_search_values", "ivfhnsw_gpu_range_search_values_dev",
    "ivfhnsw_gpu_search_tags_values", "ivfhnsw_gpu_search_tags_values_dev",
    "ivfhnsw_gpu_range_search_tags_values", "ivfhnsw_gpu_range_search_tags_values_dev", "ivfhnsw_gpu_tag_value_rows",
    "ivfhnsw_gpu_set_base_tags", "ivfhnsw_gpu_set_base_tags_dev", "ivfhnsw_gpu_clear_base_tags",
    "ivfhnsw_gpu_base_tags_info", "ivfhnsw_gpu_base_tag_rows",
    "ivfhnsw_gpu_exact_search_tags", "ivfhnsw_gpu_exact_search_tags_dev",
    "ivfhnsw_gpu_exact_range_search_tags", "ivfhnsw_gpu_exact_range_search_tags_dev",
    "ivfhnsw_gpu_set_base_values", "ivfhnsw_gpu_set_base_values_dev", "ivfhnsw_gpu_clear_base_values",
    "ivfhnsw_gpu_base_values_info", "ivfhnsw_gpu_base_value_rows",
    "ivfhnsw_gpu_exact_search_values", "ivfhnsw_gpu_exact_search_values_dev",
    "ivfhnsw_gpu_exact_range_search_values", "ivfhnsw_gpu_exact_range_search_values_dev",
    "ivfhnsw_gpu_upsert_ivf", "ivfhnsw_gpu_upsert_ivf_dev", "ivfhnsw_gpu_upsert", "ivfhnsw_gpu_upsert_dev",
)


class IvfDesc(C.Structure):
    _fields_ = [("d", C.c_size_t), ("nc", C.c_size_t), ("code_size", C.c_size_t),
                ("offsets", C.c_void_p), ("ids", C.c_void_p), ("codes", C.c_void_p),
                ("norm_codes", C.c_void_p), ("centroid_norms", C.c_void_p), ("pq_centroids", C.c_void_p),
                ("norm_table", C.c_void_p), ("opq_A", C.c_void_p),
                ("shard_rank", C.c_uint32), ("shard_world", C.c_uint32), ("list_owner", C.c_void_p)]


class SearchParams(C.Structure):
    _fields_ = [("nprobe", C.c_size_t), ("max_codes", C.c_size_t), ("efSearch", C.c_size_t),
                ("do_pruning", C.c_int), ("heap_order", C.c_int)]


class IvfHnswError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("ivfhnsw_gpu error %d: %s" % (code, msg))
        self.code = code


_lib = None


def lib():
    """Load the C-ABI library (once).  Raises if it has not been built: there is no other path."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("%s not built: run __graft_entry__.build() (make -C ivf-hnsw_amd/csrc)" % LIB_PATH)
        # PyTorch-ROCm bundles its own libamdhip64.so.7; one process must not initialise two HIP runtimes
        # (torch then reports "No HIP GPUs are available").  Loading torch first makes this library bind to
        # the runtime torch uses, whichever of the two the caller touches first afterwards.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(LIB_PATH)
        L.ivfhnsw_gpu_last_error.restype = C.c_char_p
        L.ivfhnsw_gpu_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
        L.ivfhnsw_gpu_create_view.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
        L.ivfhnsw_gpu_destroy.argtypes = [C.c_void_p]
        L.ivfhnsw_gpu_set_stream.argtypes = [C.c_void_p, C.c_void_p]
        L.ivfhnsw_gpu_sync.argtypes = [C.c_void_p]
        L.ivfhnsw_gpu_upload_ivf.argtypes = [C.c_void_p, C.POINTER(IvfDesc)]
        L.ivfhnsw_gpu_upload_ivf_synthetic.argtypes = [C.c_void_p, C.POINTER(IvfDesc), C.c_uint64]
        L.ivfhnsw_gpu_upload_grouping.argtypes = [C.c_void_p, C.c_size_t] + [C.c_void_p] * 4
        L.ivfhnsw_gpu_upload_quantizer.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_uint32,
                                                   C.c_void_p, C.c_void_p, C.c_void_p]
        L.ivfhnsw_gpu_search.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.POINTER(SearchParams), C.c_void_p, C.c_void_p]
        L.ivfhnsw_gpu_search_dev.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.POINTER(SearchParams), C.c_void_p, C.c_void_p, C.c_void_p]
        L.ivfhnsw_gpu_resolve_keys_dev.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p,
                                                   C.c_void_p]
        L.ivfhnsw_gpu_coarse_dev.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p,
                                             C.c_void_p]
        L.ivfhnsw_gpu_coarse.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p,
                                         C.c_void_p]
        L.ivfhnsw_gpu_upload_codebooks.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
        L.ivfhnsw_gpu_encode.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                                         C.c_void_p, C.c_void_p]
        L.ivfhnsw_gpu_encode_groups.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p,
                                                C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.ivfhnsw_gpu_rotate_dev.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        L.ivfhnsw_gpu_set_profiling.argtypes = [C.c_void_p, C.c_int]
        L.ivfhnsw_gpu_get_stage_ms.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
        L.ivfhnsw_gpu_reset_stage_ms.argtypes = [C.c_void_p]
        L.ivfhnsw_gpu_last_scan_counts.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.ivfhnsw_gpu_memory_bytes.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
        L.ivfhnsw_gpu_last_stream_dev.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p,
                                                  C.POINTER(C.c_uint32)]
        L.ivfhnsw_gpu_replay_stream_dev.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_uint32,
                                                    C.c_void_p]
        L.ivfhnsw_gpu_pq_train.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_void_p, C.c_size_t,
                                           C.c_void_p, C.c_void_p]
        L.ivfhnsw_gpu_xty.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
        L.ivfhnsw_gpu_kmeans.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_void_p, C.c_size_t,
                                         C.c_void_p, C.c_void_p, C.c_void_p]
        L.ivfhnsw_gpu_kmeans_dev.argtypes = L.ivfhnsw_gpu_kmeans.argtypes
        L.ivfhnsw_gpu_append_ivf.argtypes = [C.c_void_p, C.c_size_t] + [C.c_void_p] * 4
        L.ivfhnsw_gpu_append_ivf_dev.argtypes = L.ivfhnsw_gpu_append_ivf.argtypes
        L.ivfhnsw_gpu_add.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t] + [C.c_void_p] * 4
        L.ivfhnsw_gpu_add_dev.argtypes = L.ivfhnsw_gpu_add.argtypes
        L.ivfhnsw_gpu_download_ivf.argtypes = [C.c_void_p] + [C.c_void_p] * 4
        L.ivfhnsw_gpu_remove_ids.argtypes = [C.c_void_p, C.c_size_t] + [C.c_void_p] * 3
        L.ivfhnsw_gpu_remove_ids_dev.argtypes = L.ivfhnsw_gpu_remove_ids.argtypes
        L.ivfhnsw_gpu_upsert_ivf.argtypes = [C.c_void_p, C.c_size_t] + [C.c_void_p] * 6
        L.ivfhnsw_gpu_upsert_ivf_dev.argtypes = L.ivfhnsw_gpu_upsert_ivf.argtypes
        L.ivfhnsw_gpu_upsert.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t] + [C.c_void_p] * 5
        L.ivfhnsw_gpu_upsert_dev.argtypes = L.ivfhnsw_gpu_upsert.argtypes
        L.ivfhnsw_gpu_download_grouping.argtypes = [C.c_void_p, C.c_void_p]
        L.ivfhnsw_gpu_append_grouping.argtypes = [C.c_void_p, C.c_size_t] + [C.c_void_p] * 5
        L.ivfhnsw_gpu_append_grouping_dev.argtypes = L.ivfhnsw_gpu_append_grouping.argtypes
        L.ivfhnsw_gpu_add_groups.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t] + \
            [C.c_void_p] * 7
        L.ivfhnsw_gpu_add_groups_dev.argtypes = L.ivfhnsw_gpu_add_groups.argtypes
        L.ivfhnsw_gpu_download_grouping_tables.argtypes = [C.c_void_p] + [C.c_void_p] * 4
        L.ivfhnsw_gpu_upload_centroid_norms.argtypes = [C.c_void_p, C.c_void_p]
        L.ivfhnsw_gpu_knn.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t,
                                      C.c_int, C.c_void_p, C.c_void_p]
        L.ivfhnsw_gpu_build_graph.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t,
                                              C.c_size_t, C.c_void_p, C.c_void_p]
        L.ivfhnsw_gpu_build_graph_dev.argtypes = L.ivfhnsw_gpu_build_graph.argtypes
        L.ivfhnsw_gpu_last_graph_longest_reverse.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
        L.ivfhnsw_gpu_knn_dev.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t,
                                          C.c_int, C.c_void_p, C.c_void_p]
        L.ivfhnsw_gpu_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_long]
        L.ivfhnsw_gpu_search_sharded.argtypes = [C.POINTER(C.c_void_p), C.c_size_t, C.c_size_t, C.c_size_t, C.c_void_p,
                                                 C.c_void_p, C.c_void_p, C.POINTER(SearchParams), C.c_void_p, C.c_void_p]
        L.ivfhnsw_gpu_prepare_latency.argtypes = [C.c_void_p]
        L.ivfhnsw_gpu_set_batch_split.argtypes = [C.c_void_p, C.c_int]
        L.ivfhnsw_gpu_last_batch_parts.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.ivfhnsw_gpu_upload_base.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_void_p,
                                              C.c_size_t]
        L.ivfhnsw_gpu_upload_base_dev.argtypes = L.ivfhnsw_gpu_upload_base.argtypes
        L.ivfhnsw_gpu_rerank_dev.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t,
                                             C.c_void_p, C.c_void_p]
        L.ivfhnsw_gpu_rerank.argtypes = L.ivfhnsw_gpu_rerank_dev.argtypes
        L.ivfhnsw_gpu_exact_search.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p,
                                               C.c_void_p]
        L.ivfhnsw_gpu_exact_search_dev.argtypes = L.ivfhnsw_gpu_exact_search.argtypes
        L.ivfhnsw_gpu_exact_range_search.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_float, C.c_void_p,
                                                     C.POINTER(C.c_uint64)]
        L.ivfhnsw_gpu_exact_range_search_dev.argtypes = L.ivfhnsw_gpu_exact_range_search.argtypes
        L.ivfhnsw_gpu_exact_range_results.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p]
        L.ivfhnsw_gpu_exact_range_results_dev.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                                          C.POINTER(C.c_uint64)]
        L.ivfhnsw_gpu_set_filter.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_int]
        L.ivfhnsw_gpu_set_filter_dev.argtypes = L.ivfhnsw_gpu_set_filter.argtypes
        L.ivfhnsw_gpu_clear_filter.argtypes = [C.c_void_p]
        L.ivfhnsw_gpu_filter_info.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.ivfhnsw_gpu_set_filter_slot.argtypes = [C.c_void_p, C.c_uint, C.c_size_t, C.c_void_p, C.c_int]
        L.ivfhnsw_gpu_set_filter_slot_dev.argtypes = L.ivfhnsw_gpu_set_filter_slot.argtypes
        L.ivfhnsw_gpu_clear_filter_slot.argtypes = [C.c_void_p, C.c_int]
        L.ivfhnsw_gpu_filter_slot_info.argtypes = [C.c_void_p, C.c_uint, C.POINTER(C.c_int), C.POINTER(C.c_uint64),
                                                   C.POINTER(C.c_uint64)]
        L.ivfhnsw_gpu_search_slots.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p,
                                               C.POINTER(SearchParams), C.c_void_p, C.c_void_p, C.c_void_p]
        L.ivfhnsw_gpu_search_slots_dev.argtypes = L.ivfhnsw_gpu_search_slots.argtypes + [C.c_void_p]
        L.ivfhnsw_gpu_range_search_slots.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p,
                                                     C.POINTER(SearchParams), C.c_void_p, C.c_float, C.c_void_p,
                                                     C.POINTER(C.c_uint64)]
        L.ivfhnsw_gpu_range_search_slots_dev.argtypes = L.ivfhnsw_gpu_range_search_slots.argtypes
        L.ivfhnsw_gpu_set_tags.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        L.ivfhnsw_gpu_set_tags_dev.argtypes = L.ivfhnsw_gpu_set_tags.argtypes
        L.ivfhnsw_gpu_clear_tags.argtypes = [C.c_void_p]
        L.ivfhnsw_gpu_tags_info.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.ivfhnsw_gpu_tag_rows.argtypes = [C.c_void_p, C.c_uint, C.POINTER(C.c_uint64)]
        L.ivfhnsw_gpu_search_tags.argtypes = L.ivfhnsw_gpu_search_slots.argtypes
        L.ivfhnsw_gpu_search_tags_dev.argtypes = L.ivfhnsw_gpu_search_slots_dev.argtypes
        L.ivfhnsw_gpu_range_search_tags.argtypes = L.ivfhnsw_gpu_range_search_slots.argtypes
        L.ivfhnsw_gpu_range_search_tags_dev.argtypes = L.ivfhnsw_gpu_range_search_slots.argtypes
        L.ivfhnsw_gpu_set_values.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        L.ivfhnsw_gpu_set_values_dev.argtypes = L.ivfhnsw_gpu_set_values.argtypes
        L.ivfhnsw_gpu_clear_values.argtypes = [C.c_void_p]
        L.ivfhnsw_gpu_values_info.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.ivfhnsw_gpu_value_rows.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64)]
        L.ivfhnsw_gpu_search_values.argtypes = L.ivfhnsw_gpu_search_slots.argtypes
        L.ivfhnsw_gpu_search_values_dev.argtypes = L.ivfhnsw_gpu_search_slots_dev.argtypes
        L.ivfhnsw_gpu_range_search_values.argtypes = L.ivfhnsw_gpu_range_search_slots.argtypes
        L.ivfhnsw_gpu_range_search_values_dev.argtypes = L.ivfhnsw_gpu_range_search_slots.argtypes
        # ... and with both arrays: the second pick pointer follows the first
        a = L.ivfhnsw_gpu_search_slots.argtypes
        L.ivfhnsw_gpu_search_tags_values.argtypes = a[:8] + [C.c_void_p] + a[8:]
        L.ivfhnsw_gpu_search_tags_values_dev.argtypes = L.ivfhnsw_gpu_search_tags_values.argtypes + [C.c_void_p]
        a = L.ivfhnsw_gpu_range_search_slots.argtypes
        L.ivfhnsw_gpu_range_search_tags_values.argtypes = a[:7] + [C.c_void_p] + a[7:]
        L.ivfhnsw_gpu_range_search_tags_values_dev.argtypes = L.ivfhnsw_gpu_range_search_tags_values.argtypes
        L.ivfhnsw_gpu_tag_value_rows.argtypes = [C.c_void_p, C.c_uint, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64)]
        L.ivfhnsw_gpu_set_base_filter.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_int]
        L.ivfhnsw_gpu_set_base_filter_dev.argtypes = L.ivfhnsw_gpu_set_base_filter.argtypes
        L.ivfhnsw_gpu_clear_base_filter.argtypes = [C.c_void_p]
        L.ivfhnsw_gpu_base_filter_info.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.ivfhnsw_gpu_set_base_filter_slot.argtypes = [C.c_void_p, C.c_uint, C.c_size_t, C.c_void_p, C.c_int]
        L.ivfhnsw_gpu_set_base_filter_slot_dev.argtypes = L.ivfhnsw_gpu_set_base_filter_slot.argtypes
        L.ivfhnsw_gpu_clear_base_filter_slot.argtypes = [C.c_void_p, C.c_int]
        L.ivfhnsw_gpu_base_filter_slot_info.argtypes = [C.c_void_p, C.c_uint, C.POINTER(C.c_int), C.POINTER(C.c_uint64),
                                                        C.POINTER(C.c_uint64)]
        L.ivfhnsw_gpu_exact_search_slots.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p,
                                                     C.c_void_p, C.c_void_p]
        L.ivfhnsw_gpu_exact_search_slots_dev.argtypes = L.ivfhnsw_gpu_exact_search_slots.argtypes
        L.ivfhnsw_gpu_exact_range_search_slots.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_float,
                                                           C.c_void_p, C.POINTER(C.c_uint64)]
        L.ivfhnsw_gpu_exact_range_search_slots_dev.argtypes = L.ivfhnsw_gpu_exact_range_search_slots.argtypes
        L.ivfhnsw_gpu_set_base_tags.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        L.ivfhnsw_gpu_set_base_tags_dev.argtypes = L.ivfhnsw_gpu_set_base_tags.argtypes
        L.ivfhnsw_gpu_clear_base_tags.argtypes = [C.c_void_p]
        L.ivfhnsw_gpu_base_tags_info.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.ivfhnsw_gpu_base_tag_rows.argtypes = [C.c_void_p, C.c_uint, C.POINTER(C.c_uint64)]
        L.ivfhnsw_gpu_exact_search_tags.argtypes = L.ivfhnsw_gpu_exact_search_slots.argtypes
        L.ivfhnsw_gpu_exact_search_tags_dev.argtypes = L.ivfhnsw_gpu_exact_search_slots.argtypes
        L.ivfhnsw_gpu_exact_range_search_tags.argtypes = L.ivfhnsw_gpu_exact_range_search_slots.argtypes
        L.ivfhnsw_gpu_exact_range_search_tags_dev.argtypes = L.ivfhnsw_gpu_exact_range_search_slots.argtypes
        L.ivfhnsw_gpu_set_base_values.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        L.ivfhnsw_gpu_set_base_values_dev.argtypes = L.ivfhnsw_gpu_set_base_values.argtypes
        L.ivfhnsw_gpu_clear_base_values.argtypes = [C.c_void_p]
        L.ivfhnsw_gpu_base_values_info.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.ivfhnsw_gpu_base_value_rows.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64)]
        L.ivfhnsw_gpu_exact_search_values.argtypes = L.ivfhnsw_gpu_exact_search_slots.argtypes
        L.ivfhnsw_gpu_exact_search_values_dev.argtypes = L.ivfhnsw_gpu_exact_search_slots.argtypes
        L.ivfhnsw_gpu_exact_range_search_values.argtypes = L.ivfhnsw_gpu_exact_range_search_slots.argtypes
        L.ivfhnsw_gpu_exact_range_search_values_dev.argtypes = L.ivfhnsw_gpu_exact_range_search_slots.argtypes
        L.ivfhnsw_gpu_range_search.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p,
                                               C.POINTER(SearchParams), C.c_float, C.c_void_p, C.POINTER(C.c_uint64)]
        L.ivfhnsw_gpu_range_search_dev.argtypes = L.ivfhnsw_gpu_range_search.argtypes
        L.ivfhnsw_gpu_range_results.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p]
        L.ivfhnsw_gpu_range_results_dev.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                                    C.POINTER(C.c_uint64)]
        L.ivfhnsw_gpu_locate.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
        L.ivfhnsw_gpu_locate_dev.argtypes = L.ivfhnsw_gpu_locate.argtypes
        L.ivfhnsw_gpu_reconstruct_rows.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p]
        L.ivfhnsw_gpu_reconstruct_rows_dev.argtypes = L.ivfhnsw_gpu_reconstruct_rows.argtypes
        L.ivfhnsw_gpu_reconstruct.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_uint64)]
        L.ivfhnsw_gpu_reconstruct_dev.argtypes = L.ivfhnsw_gpu_reconstruct.argtypes
        L.ivfhnsw_gpu_search_reconstruct.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p,
                                                     C.POINTER(SearchParams), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                                     C.c_void_p]
        L.ivfhnsw_gpu_search_reconstruct_dev.argtypes = L.ivfhnsw_gpu_search_reconstruct.argtypes
        L.ivfhnsw_gpu_last_scan_kernel.argtypes = [C.c_void_p]
        L.ivfhnsw_gpu_last_scan_kernel.restype = C.c_char_p
        _lib = L
    return _lib


def _check(rc):
    if rc != OK:
        raise IvfHnswError(rc, lib().ivfhnsw_gpu_last_error().decode())


def _np(a, dtype):
    a = np.ascontiguousarray(a, dtype=dtype)
    return a


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _devptr(t):
    """Device pointer of a torch tensor (or a raw int address / None)."""
    if t is None:
        return None
    if isinstance(t, int):
        return C.c_void_p(t)
    assert t.is_cuda and t.is_contiguous()
    return C.c_void_p(t.data_ptr())


def search_sharded(shards, queries, k, nprobe, max_codes, coarse_ids, coarse_dists, do_pruning=False):
    """ivfhnsw_gpu_search_sharded: the shard step over all shard handles of one process (RCCL merge across devices, host
    merge when they share one); host arrays in and out."""
    q = _np(queries, np.float32)
    q = q.reshape(-1, q.shape[-1])
    nq = q.shape[0]
    cid = _np(coarse_ids, np.uint32).reshape(nq, nprobe)
    cd = _np(coarse_dists, np.float32).reshape(nq, nprobe)
    dist = np.empty((nq, k), np.float32)
    lab = np.empty((nq, k), np.int64)
    arr = (C.c_void_p * len(shards))(*[g._h for g in shards])
    p = SearchParams(nprobe, max_codes, 0, 1 if do_pruning else 0, 0)
    _check(lib().ivfhnsw_gpu_search_sharded(arr, len(shards), nq, k, _ptr(q), _ptr(cid), _ptr(cd), C.byref(p), _ptr(dist),
                                            _ptr(lab)))
    return dist, lab


class GpuIndex:
    """One device-side index (ivfhnsw_gpu handle)."""

    def __init__(self, device=0):
        self._h = C.c_void_p()
        self._device = device
        _check(lib().ivfhnsw_gpu_create(device, C.byref(self._h)))
        self.d = self.nc = self.code_size = 0

    def view(self):
        """A second search context on this index's device tables (own stream and workspace; nothing copied).
        Keep this object alive, and do not upload to it, while the view is in use."""
        v = GpuIndex.__new__(GpuIndex)
        v._h = C.c_void_p()
        _check(lib().ivfhnsw_gpu_create_view(self._h, C.byref(v._h)))
        v.d, v.nc, v.code_size = self.d, self.nc, self.code_size
        v._device = self._device
        v._parent = self
        v._shard = getattr(self, "_shard", (0, 1, None))
        v._nsubc = getattr(self, "_nsubc", 0)
        return v

    def close(self):
        if self._h:
            lib().ivfhnsw_gpu_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- uploads -------------------------------------------------------------------------------
    def _desc(self, d, code_size, offsets, centroid_norms, pq_centroids, norm_table, opq_A, ids, codes, norm_codes,
              shard_rank, shard_world, list_owner=None):
        keep = {}
        keep["offsets"] = _np(offsets, np.uint64)
        nc = len(keep["offsets"]) - 1
        keep["centroid_norms"] = _np(centroid_norms, np.float32)
        keep["pq_centroids"] = _np(pq_centroids, np.float32)
        keep["norm_table"] = _np(norm_table, np.float32)
        assert keep["centroid_norms"].size == nc
        assert keep["pq_centroids"].size == 256 * d
        assert keep["norm_table"].size == 256
        keep["opq_A"] = None if opq_A is None else _np(opq_A, np.float32)
        keep["ids"] = None if ids is None else _np(ids, np.uint32)
        keep["codes"] = None if codes is None else _np(codes, np.uint8)
        keep["norm_codes"] = None if norm_codes is None else _np(norm_codes, np.uint8)
        keep["list_owner"] = None if list_owner is None else _np(list_owner, np.uint32)
        assert keep["list_owner"] is None or keep["list_owner"].size == nc
        desc = IvfDesc(d, nc, code_size, _ptr(keep["offsets"]), _ptr(keep["ids"]), _ptr(keep["codes"]),
                       _ptr(keep["norm_codes"]), _ptr(keep["centroid_norms"]), _ptr(keep["pq_centroids"]),
                       _ptr(keep["norm_table"]), _ptr(keep["opq_A"]), shard_rank, shard_world,
                       _ptr(keep["list_owner"]))
        self.d, self.nc, self.code_size = d, nc, code_size
        self._shard = (shard_rank, shard_world, keep["list_owner"])
        return desc, keep

    def upload_ivf(self, d, code_size, offsets, ids, codes, norm_codes, centroid_norms, pq_centroids, norm_table,
                   opq_A=None, shard_rank=0, shard_world=1, list_owner=None):
        desc, keep = self._desc(d, code_size, offsets, centroid_norms, pq_centroids, norm_table, opq_A, ids, codes,
                                norm_codes, shard_rank, shard_world, list_owner)
        _check(lib().ivfhnsw_gpu_upload_ivf(self._h, C.byref(desc)))

    def upload_ivf_synthetic(self, d, code_size, offsets, centroid_norms, pq_centroids, norm_table, seed, opq_A=None,
                             shard_rank=0, shard_world=1, list_owner=None):
        desc, keep = self._desc(d, code_size, offsets, centroid_norms, pq_centroids, norm_table, opq_A, None, None,
                                None, shard_rank, shard_world, list_owner)
        _check(lib().ivfhnsw_gpu_upload_ivf_synthetic(self._h, C.byref(desc), seed))

    # ---- appends (ivfhnsw_gpu_append_ivf / ivfhnsw_gpu_add) -------------------------------------
    def append_ivf(self, list_idx, ids, codes, norm_codes):
        """Append code i to the end of list list_idx[i] (IndexIVF_HNSW.cpp:122-131) in HBM; host arrays."""
        li = _np(list_idx, np.uint32).ravel()
        n = li.size
        i = _np(ids, np.uint32).ravel()
        c = _np(codes, np.uint8).reshape(n, -1) if n else np.zeros((0, self.code_size), np.uint8)
        nc = _np(norm_codes, np.uint8).ravel()
        assert i.size == n and nc.size == n and (not self.code_size or c.shape[1] == self.code_size)
        _check(lib().ivfhnsw_gpu_append_ivf(self._h, n, _ptr(li), _ptr(i), _ptr(c), _ptr(nc)))

    def append_ivf_dev(self, n, d_list_idx, d_ids, d_codes, d_norm_codes):
        """The same on device buffers (torch CUDA tensors or raw addresses)."""
        _check(lib().ivfhnsw_gpu_append_ivf_dev(self._h, n, _devptr(d_list_idx), _devptr(d_ids), _devptr(d_codes),
                                                _devptr(d_norm_codes)))

    def add(self, x, ids, precomputed_idx=None, efSearch=0):
        """encode + append_ivf without the codes leaving HBM: returns (idx, codes, norm_codes) as encode does."""
        x = _np(x, np.float32)
        x = x.reshape(-1, x.shape[-1])
        n = x.shape[0]
        i = _np(ids, np.uint32).ravel()
        assert i.size == n
        pidx = None if precomputed_idx is None else _np(precomputed_idx, np.uint32)
        idx = np.empty(n, np.uint32)
        codes = np.empty((n, self.code_size), np.uint8)
        ncodes = np.empty(n, np.uint8)
        _check(lib().ivfhnsw_gpu_add(self._h, n, _ptr(x), _ptr(pidx), efSearch, _ptr(i), _ptr(idx), _ptr(codes),
                                     _ptr(ncodes)))
        return idx, codes, ncodes

    def add_dev(self, n, d_x, d_ids, d_precomputed_idx=None, efSearch=0, d_out_idx=None, d_out_codes=None,
                d_out_norm_codes=None):
        """add on device buffers (outputs optional)."""
        _check(lib().ivfhnsw_gpu_add_dev(self._h, n, _devptr(d_x), _devptr(d_precomputed_idx), efSearch, _devptr(d_ids),
                                         _devptr(d_out_idx), _devptr(d_out_codes), _devptr(d_out_norm_codes)))

    def download_ivf(self):
        """(offsets u64 [nc+1], ids u32 [n_local], codes u8 [n_local, code_size], norm_codes u8 [n_local]) as the
        handle holds them: this shard's lists only, in the layout upload_ivf takes."""
        off = np.empty(self.nc + 1, np.uint64)
        _check(lib().ivfhnsw_gpu_download_ivf(self._h, _ptr(off), None, None, None))
        rank, world, owner = getattr(self, "_shard", (0, 1, None))
        lens = np.diff(off)
        if world > 1:
            own = (owner if owner is not None else np.arange(self.nc) % world) == rank
            lens = lens[own]
        n = int(lens.sum())
        ids = np.empty(n, np.uint32)
        codes = np.empty((n, self.code_size), np.uint8)
        ncodes = np.empty(n, np.uint8)
        _check(lib().ivfhnsw_gpu_download_ivf(self._h, None, _ptr(ids), _ptr(codes), _ptr(ncodes)))
        return off, ids, codes, ncodes

    # ---- removals (ivfhnsw_gpu_remove_ids) -------------------------------------------------------
    def remove_ids(self, labels):
        """Remove every code whose id is one of `labels` from the lists in HBM (faiss remove_ids): returns (n_removed,
        removed_per_list uint32 [nc])."""
        lab = _np(labels, np.uint32).ravel()
        nr = C.c_uint64(0)
        per = np.zeros(self.nc, np.uint32)
        _check(lib().ivfhnsw_gpu_remove_ids(self._h, lab.size, _ptr(lab) if lab.size else None, C.byref(nr), _ptr(per)))
        return int(nr.value), per

    def remove_ids_dev(self, n, d_labels, d_removed_per_list=None):
        """The same on device buffers (torch CUDA tensors or raw addresses); returns n_removed."""
        nr = C.c_uint64(0)
        _check(lib().ivfhnsw_gpu_remove_ids_dev(self._h, n, _devptr(d_labels), C.byref(nr), _devptr(d_removed_per_list)))
        return int(nr.value)

    # ---- upserts (ivfhnsw_gpu_upsert_ivf / ivfhnsw_gpu_upsert) -----------------------------------
    def upsert_ivf(self, list_idx, ids, codes, norm_codes):
        """remove_ids(ids) + append_ivf(list_idx, ids, codes, norm_codes) as one atomic call that moves the lists once;
        a label twice in `ids` is an error.  Returns (n_removed, removed_per_list uint32 [nc])."""
        li = _np(list_idx, np.uint32).ravel()
        n = li.size
        i = _np(ids, np.uint32).ravel()
        c = _np(codes, np.uint8).reshape(n, -1) if n else np.zeros((0, self.code_size), np.uint8)
        nc = _np(norm_codes, np.uint8).ravel()
        assert i.size == n and nc.size == n and (not self.code_size or c.shape[1] == self.code_size)
        nr = C.c_uint64(0)
        per = np.zeros(self.nc, np.uint32)
        _check(lib().ivfhnsw_gpu_upsert_ivf(self._h, n, _ptr(li), _ptr(i), _ptr(c), _ptr(nc), C.byref(nr), _ptr(per)))
        return int(nr.value), per

    def upsert_ivf_dev(self, n, d_list_idx, d_ids, d_codes, d_norm_codes, d_removed_per_list=None):
        """The same on device buffers (torch CUDA tensors or raw addresses); returns n_removed."""
        nr = C.c_uint64(0)
        _check(lib().ivfhnsw_gpu_upsert_ivf_dev(self._h, n, _devptr(d_list_idx), _devptr(d_ids), _devptr(d_codes),
                                                _devptr(d_norm_codes), C.byref(nr), _devptr(d_removed_per_list)))
        return int(nr.value)

    def upsert(self, x, ids, precomputed_idx=None, efSearch=0):
        """encode + upsert_ivf without the codes leaving HBM: returns (idx, codes, norm_codes, n_removed)."""
        x = _np(x, np.float32)
        x = x.reshape(-1, x.shape[-1])
        n = x.shape[0]
        i = _np(ids, np.uint32).ravel()
        assert i.size == n
        pidx = None if precomputed_idx is None else _np(precomputed_idx, np.uint32)
        idx = np.empty(n, np.uint32)
        codes = np.empty((n, self.code_size), np.uint8)
        ncodes = np.empty(n, np.uint8)
        nr = C.c_uint64(0)
        _check(lib().ivfhnsw_gpu_upsert(self._h, n, _ptr(x), _ptr(pidx), efSearch, _ptr(i), _ptr(idx), _ptr(codes),
                                        _ptr(ncodes), C.byref(nr)))
        return idx, codes, ncodes, int(nr.value)

    def upsert_dev(self, n, d_x, d_ids, d_precomputed_idx=None, efSearch=0, d_out_idx=None, d_out_codes=None,
                   d_out_norm_codes=None):
        """upsert on device buffers (outputs optional); returns n_removed."""
        nr = C.c_uint64(0)
        _check(lib().ivfhnsw_gpu_upsert_dev(self._h, n, _devptr(d_x), _devptr(d_precomputed_idx), efSearch, _devptr(d_ids),
                                            _devptr(d_out_idx), _devptr(d_out_codes), _devptr(d_out_norm_codes),
                                            C.byref(nr)))
        return int(nr.value)

    # ---- label filter (ivfhnsw_gpu_set_filter) ---------------------------------------------------
    def set_filter(self, labels, deny=False):
        """Searches return only rows whose id is in `labels` (deny=True: is not in them); replaces an earlier filter."""
        lab = _np(labels, np.uint32).ravel()
        _check(lib().ivfhnsw_gpu_set_filter(self._h, lab.size, _ptr(lab) if lab.size else None,
                                            FILTER_DENY if deny else FILTER_ALLOW))

    def set_filter_dev(self, n, d_labels, deny=False):
        """The same on a device buffer (torch CUDA tensor or raw address)."""
        _check(lib().ivfhnsw_gpu_set_filter_dev(self._h, n, _devptr(d_labels), FILTER_DENY if deny else FILTER_ALLOW))

    def clear_filter(self):
        _check(lib().ivfhnsw_gpu_clear_filter(self._h))

    def filter_info(self):
        """(mode or -1, rows_passing, rows_total)."""
        m, a, b = C.c_int(-1), C.c_uint64(0), C.c_uint64(0)
        _check(lib().ivfhnsw_gpu_filter_info(self._h, C.byref(m), C.byref(a), C.byref(b)))
        return int(m.value), int(a.value), int(b.value)

    # ---- filter slots: a label filter per query (ivfhnsw_gpu_set_filter_slot) -----------------------
    def set_filter_slot(self, slot, labels, deny=False):
        """Slot `slot` (0..FILTER_SLOTS-1) holds the set `labels`, allow or deny as set_filter; replaces the slot's earlier
        set.  The _slots searches name a slot per query."""
        lab = _np(labels, np.uint32).ravel()
        _check(lib().ivfhnsw_gpu_set_filter_slot(self._h, slot, lab.size, _ptr(lab) if lab.size else None,
                                                 FILTER_DENY if deny else FILTER_ALLOW))

    def set_filter_slot_dev(self, slot, n, d_labels, deny=False):
        """The same on a device buffer (torch CUDA tensor or raw address)."""
        _check(lib().ivfhnsw_gpu_set_filter_slot_dev(self._h, slot, n, _devptr(d_labels),
                                                     FILTER_DENY if deny else FILTER_ALLOW))

    def clear_filter_slot(self, slot=None):
        """The slot passes nothing afterwards; None: every slot."""
        _check(lib().ivfhnsw_gpu_clear_filter_slot(self._h, -1 if slot is None else slot))

    def filter_slot_info(self, slot):
        """(mode or -1, rows_passing, rows_total) of one slot."""
        m, a, b = C.c_int(-1), C.c_uint64(0), C.c_uint64(0)
        _check(lib().ivfhnsw_gpu_filter_slot_info(self._h, slot, C.byref(m), C.byref(a), C.byref(b)))
        return int(m.value), int(a.value), int(b.value)

    # ---- row tags: disjoint sets as a 16-bit tag per row (ivfhnsw_gpu_set_tags) -------------------------
    def set_tags(self, labels, tags):
        """The labels given carry the tags given (uint16; TAG_NONE untags) from now on; every other label keeps its tag.
        The _tags searches name a tag per query."""
        lab = _np(labels, np.uint32).ravel()
        tg = _np(tags, np.uint16).ravel()
        if tg.size != lab.size:
            raise ValueError("set_tags: %d labels, %d tags" % (lab.size, tg.size))
        _check(lib().ivfhnsw_gpu_set_tags(self._h, lab.size, _ptr(lab) if lab.size else None, _ptr(tg) if tg.size else None))

    def set_tags_dev(self, n, d_labels, d_tags):
        """The same on device buffers (torch CUDA tensors or raw addresses)."""
        _check(lib().ivfhnsw_gpu_set_tags_dev(self._h, n, _devptr(d_labels), _devptr(d_tags)))

    def clear_tags(self):
        """No label is tagged afterwards."""
        _check(lib().ivfhnsw_gpu_clear_tags(self._h))

    def tags_info(self):
        """(rows_tagged, rows_total, table_labels): resident rows with a tag, resident rows, label values the table spans."""
        a, b, c = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        _check(lib().ivfhnsw_gpu_tags_info(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return int(a.value), int(b.value), int(c.value)

    def tag_rows(self, tag):
        """Resident rows that carry `tag`."""
        n = C.c_uint64(0)
        _check(lib().ivfhnsw_gpu_tag_rows(self._h, tag, C.byref(n)))
        return int(n.value)

    # ---- row values: a uint32 per row, an interval per query (ivfhnsw_gpu_set_values) ------------------
    def set_values(self, labels, values):
        """The labels given carry the values given (uint32; VALUE_NONE un-values) from now on; every other label keeps
        its value.  The _values searches name an interval per query."""
        lab = _np(labels, np.uint32).ravel()
        vl = _np(values, np.uint32).ravel()
        if vl.size != lab.size:
            raise ValueError("set_values: %d labels, %d values" % (lab.size, vl.size))
        _check(lib().ivfhnsw_gpu_set_values(self._h, lab.size, _ptr(lab) if lab.size else None, _ptr(vl) if vl.size else None))

    def set_values_dev(self, n, d_labels, d_values):
        """The same on device buffers (torch CUDA tensors or raw addresses)."""
        _check(lib().ivfhnsw_gpu_set_values_dev(self._h, n, _devptr(d_labels), _devptr(d_values)))

    def clear_values(self):
        """No label has a value afterwards."""
        _check(lib().ivfhnsw_gpu_clear_values(self._h))

    def values_info(self):
        """(rows_valued, rows_total, table_labels): resident rows with a value, resident rows, label values the table spans."""
        a, b, c = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        _check(lib().ivfhnsw_gpu_values_info(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return int(a.value), int(b.value), int(c.value)

    def value_rows(self, lo, hi):
        """Resident rows whose value lies in [lo, hi], unsigned and inclusive; a row without a value holds VALUE_NONE."""
        n = C.c_uint64(0)
        _check(lib().ivfhnsw_gpu_value_rows(self._h, lo, hi, C.byref(n)))
        return int(n.value)

    # ---- row tags AND row values: both per query (ivfhnsw_gpu_search_tags_values) -----------------------
    def tag_value_rows(self, tag, lo, hi):
        """Resident rows whose tag passes `tag` (TAG_NONE: every row) AND whose value lies in [lo, hi]."""
        n = C.c_uint64(0)
        _check(lib().ivfhnsw_gpu_tag_value_rows(self._h, tag, lo, hi, C.byref(n)))
        return int(n.value)

    def upload_grouping(self, nsubc, alphas, nn_centroid_idxs, subgroup_sizes, inter_centroid_dists):
        a = _np(alphas, np.float32)
        n = _np(nn_centroid_idxs, np.uint32)
        s = _np(subgroup_sizes, np.uint32)
        i = _np(inter_centroid_dists, np.float32)
        assert a.size == self.nc and n.size == s.size == i.size == self.nc * nsubc
        _check(lib().ivfhnsw_gpu_upload_grouping(self._h, nsubc, _ptr(a), _ptr(n), _ptr(s), _ptr(i)))
        self._nsubc = nsubc

    def download_grouping(self):
        """The sub-group sizes the handle holds, uint32 [nc, nsubc] as upload_grouping takes them."""
        out = np.empty((self.nc, getattr(self, "_nsubc", 0)), np.uint32)
        _check(lib().ivfhnsw_gpu_download_grouping(self._h, _ptr(out) if out.size else None))
        return out

    # ---- additions to a Grouping index (ivfhnsw_gpu_append_grouping / ivfhnsw_gpu_add_groups) ----
    def append_grouping(self, list_idx, sub_idx, ids, codes, norm_codes):
        """Put code i at the end of sub-group sub_idx[i] of list list_idx[i] (IndexIVF_HNSW_Grouping.cpp:127-155) in HBM;
        host arrays."""
        li = _np(list_idx, np.uint32).ravel()
        n = li.size
        si = _np(sub_idx, np.uint32).ravel()
        i = _np(ids, np.uint32).ravel()
        c = _np(codes, np.uint8).reshape(n, -1) if n else np.zeros((0, self.code_size), np.uint8)
        nc = _np(norm_codes, np.uint8).ravel()
        assert si.size == n and i.size == n and nc.size == n and (not self.code_size or c.shape[1] == self.code_size)
        _check(lib().ivfhnsw_gpu_append_grouping(self._h, n, _ptr(li), _ptr(si), _ptr(i), _ptr(c), _ptr(nc)))

    def append_grouping_dev(self, n, d_list_idx, d_sub_idx, d_ids, d_codes, d_norm_codes):
        """The same on device buffers (torch CUDA tensors or raw addresses)."""
        _check(lib().ivfhnsw_gpu_append_grouping_dev(self._h, n, _devptr(d_list_idx), _devptr(d_sub_idx), _devptr(d_ids),
                                                     _devptr(d_codes), _devptr(d_norm_codes)))

    def add_groups(self, centroid_idx, offsets, x, ids, efSearch, inter_centroid_dists=None, alphas_in=None):
        """add_group for groups that hold no codes: encode_groups + the install of rows and codes in HBM.  Returns what
        encode_groups does: (nn_centroid_idxs [G, nsubc], alphas [G], subcentroid_idxs [n], codes [n, M], norm_codes [n]).
        inter_centroid_dists None: the rows are computed on the device; [G, nsubc]: stored as given."""
        cidx = _np(centroid_idx, np.uint32).ravel()
        off = _np(offsets, np.uint64).ravel()
        G = cidx.size
        nsubc = getattr(self, "_nsubc", 0)
        x = _np(x, np.float32)
        x = x.reshape(-1, x.shape[-1]) if x.size else x.reshape(0, 1)
        n = int(off[-1]) if off.size else 0
        i = _np(ids, np.uint32).ravel()
        assert off.size == G + 1 and i.size == n and x.shape[0] == n
        icd = None if inter_centroid_dists is None else _np(inter_centroid_dists, np.float32)
        assert icd is None or icd.size == G * nsubc
        nn = np.empty((G, nsubc), np.uint32)
        alphas = np.zeros(G, np.float32) if alphas_in is None else _np(alphas_in, np.float32).copy()
        sub = np.empty(n, np.uint32)
        codes = np.empty((n, self.code_size), np.uint8)
        ncodes = np.empty(n, np.uint8)
        _check(lib().ivfhnsw_gpu_add_groups(self._h, G, _ptr(cidx), _ptr(off), _ptr(x), efSearch, _ptr(i), _ptr(icd),
                                            _ptr(nn), _ptr(alphas), _ptr(sub), _ptr(codes), _ptr(ncodes)))
        return nn, alphas, sub, codes, ncodes

    def add_groups_dev(self, ngroups, d_centroid_idx, d_offsets, d_x, d_ids, efSearch, d_out_nn_centroid_idxs, d_out_alphas,
                       d_out_subcentroid_idxs, d_out_codes, d_out_norm_codes=None, d_inter_centroid_dists=None):
        """add_groups on device buffers (d_offsets uint64 [ngroups + 1]; d_out_norm_codes optional)."""
        _check(lib().ivfhnsw_gpu_add_groups_dev(self._h, ngroups, _devptr(d_centroid_idx), _devptr(d_offsets), _devptr(d_x),
                                                efSearch, _devptr(d_ids), _devptr(d_inter_centroid_dists),
                                                _devptr(d_out_nn_centroid_idxs), _devptr(d_out_alphas),
                                                _devptr(d_out_subcentroid_idxs), _devptr(d_out_codes),
                                                _devptr(d_out_norm_codes)))

    def download_grouping_tables(self):
        """(alphas f32 [nc], nn_centroid_idxs u32 [nc, nsubc], subgroup_sizes u32 [nc, nsubc], inter_centroid_dists f32
        [nc, nsubc]) as the handle holds them."""
        nsubc = getattr(self, "_nsubc", 0)
        a = np.empty(self.nc, np.float32)
        nn = np.empty((self.nc, nsubc), np.uint32)
        sz = np.empty((self.nc, nsubc), np.uint32)
        icd = np.empty((self.nc, nsubc), np.float32)
        has = nsubc > 0
        _check(lib().ivfhnsw_gpu_download_grouping_tables(self._h, _ptr(a), _ptr(nn) if has else None,
                                                          _ptr(sz) if has else None, _ptr(icd) if has else None))
        return a, nn, sz, icd

    def upload_centroid_norms(self, centroid_norms):
        """Replace the [nc] centroid norms upload_ivf brought (compute_centroid_norms) and nothing else."""
        cn = _np(centroid_norms, np.float32).ravel()
        assert cn.size == self.nc
        _check(lib().ivfhnsw_gpu_upload_centroid_norms(self._h, _ptr(cn)))

    def upload_quantizer(self, link_counts, links, vectors, enterpoint=0):
        c = _np(link_counts, np.uint8)
        v = _np(vectors, np.float32)
        n, d = v.shape
        l = _np(links, np.uint32).reshape(n, -1)
        _check(lib().ivfhnsw_gpu_upload_quantizer(self._h, n, d, l.shape[1], enterpoint, _ptr(c), _ptr(l), _ptr(v)))

    def prepare_latency(self):
        """Build the fat graph of the latency walk (one query per call; see ivfhnsw_gpu_prepare_latency)."""
        _check(lib().ivfhnsw_gpu_prepare_latency(self._h))

    def set_batch_split(self, permille):
        """Batches of >= 8192 queries as two uneven parts on two streams (ivfhnsw_gpu_set_batch_split); 0 = off,
        1..999 = the first part's share, 1000 = chosen per call (the default)."""
        _check(lib().ivfhnsw_gpu_set_batch_split(self._h, int(permille)))

    def last_batch_parts(self):
        """(first, second): queries in the two parts of the last search call; second = 0 when it ran in one part."""
        a, b = C.c_uint64(0), C.c_uint64(0)
        _check(lib().ivfhnsw_gpu_last_batch_parts(self._h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    # ---- search --------------------------------------------------------------------------------
    @staticmethod
    def _params(nprobe, max_codes, efSearch, do_pruning, heap_order=False):
        return SearchParams(nprobe, max_codes, efSearch, 1 if do_pruning else 0, 1 if heap_order else 0)

    def search(self, queries, k, nprobe, max_codes, coarse_ids=None, coarse_dists=None, efSearch=0,
               do_pruning=False, heap_order=False):
        """Host arrays in, host arrays out (ivfhnsw_gpu_search)."""
        q = _np(queries, np.float32)
        q = q.reshape(-1, self.d or q.shape[-1])  # before any upload the library itself refuses the call
        nq = q.shape[0]
        cid = None if coarse_ids is None else _np(coarse_ids, np.uint32).reshape(nq, nprobe)
        cd = None if coarse_dists is None else _np(coarse_dists, np.float32).reshape(nq, nprobe)
        dist = np.empty((nq, k), np.float32)
        lab = np.empty((nq, k), np.int64)
        p = self._params(nprobe, max_codes, efSearch, do_pruning, heap_order)
        _check(lib().ivfhnsw_gpu_search(self._h, nq, k, _ptr(q), _ptr(cid), _ptr(cd), C.byref(p), _ptr(dist),
                                        _ptr(lab)))
        return dist, lab

    def search_dev(self, nq, k, d_queries, d_distances, d_labels, nprobe, max_codes, d_coarse_ids=None,
                   d_coarse_dists=None, efSearch=0, do_pruning=False, d_out_keys=None, heap_order=False):
        """Device buffers (torch CUDA tensors), asynchronous on the handle's stream."""
        p = self._params(nprobe, max_codes, efSearch, do_pruning, heap_order)
        _check(lib().ivfhnsw_gpu_search_dev(self._h, nq, k, _devptr(d_queries), _devptr(d_coarse_ids),
                                            _devptr(d_coarse_dists), C.byref(p), _devptr(d_distances),
                                            _devptr(d_labels), _devptr(d_out_keys)))

    def search_slots(self, queries, k, query_slots, nprobe, max_codes, coarse_ids=None, coarse_dists=None, efSearch=0,
                     do_pruning=False, heap_order=False):
        """search() with a filter slot per query: query_slots [nq] bytes, each a slot or SLOT_NONE (no filter); None is
        search() itself (ivfhnsw_gpu_search_slots)."""
        return self._search_picked(lib().ivfhnsw_gpu_search_slots, np.uint8, queries, k, query_slots, nprobe, max_codes,
                                   coarse_ids, coarse_dists, efSearch, do_pruning, heap_order)

    def search_tags(self, queries, k, query_tags, nprobe, max_codes, coarse_ids=None, coarse_dists=None, efSearch=0,
                    do_pruning=False, heap_order=False):
        """search() with a row tag per query: query_tags [nq] uint16, each a tag or TAG_NONE (no filter); None is
        search() itself (ivfhnsw_gpu_search_tags)."""
        return self._search_picked(lib().ivfhnsw_gpu_search_tags, np.uint16, queries, k, query_tags, nprobe, max_codes,
                                   coarse_ids, coarse_dists, efSearch, do_pruning, heap_order)

    def search_values(self, queries, k, query_ranges, nprobe, max_codes, coarse_ids=None, coarse_dists=None, efSearch=0,
                      do_pruning=False, heap_order=False):
        """search() with a value interval per query: query_ranges [nq, 2] uint32, (lo, hi) inclusive, (0, VALUE_NONE) =
        no filter; None is search() itself (ivfhnsw_gpu_search_values)."""
        return self._search_picked(lib().ivfhnsw_gpu_search_values, np.uint32, queries, k, query_ranges, nprobe, max_codes,
                                   coarse_ids, coarse_dists, efSearch, do_pruning, heap_order, per=2)

    def search_tags_values(self, queries, k, query_tags, query_ranges, nprobe, max_codes, coarse_ids=None, coarse_dists=None,
                           efSearch=0, do_pruning=False, heap_order=False):
        """search() with a row tag AND a value interval per query (query_tags as search_tags, query_ranges as
        search_values take them): a row passes iff it passes both.  query_tags None is search_values, query_ranges None
        search_tags, both None search() itself (ivfhnsw_gpu_search_tags_values)."""
        q = _np(queries, np.float32)
        q = q.reshape(-1, self.d or q.shape[-1])
        nq = q.shape[0]
        cid = None if coarse_ids is None else _np(coarse_ids, np.uint32).reshape(nq, nprobe)
        cd = None if coarse_dists is None else _np(coarse_dists, np.float32).reshape(nq, nprobe)
        qt = None if query_tags is None else _np(query_tags, np.uint16).reshape(nq)
        qr = None if query_ranges is None else _np(query_ranges, np.uint32).reshape(nq * 2)
        dist = np.empty((nq, k), np.float32)
        lab = np.empty((nq, k), np.int64)
        p = self._params(nprobe, max_codes, efSearch, do_pruning, heap_order)
        _check(lib().ivfhnsw_gpu_search_tags_values(self._h, nq, k, _ptr(q), _ptr(cid), _ptr(cd), C.byref(p), _ptr(qt), _ptr(qr),
                                                    _ptr(dist), _ptr(lab)))
        return dist, lab

    def _search_picked(self, fn, pick_dtype, queries, k, query_slots, nprobe, max_codes, coarse_ids, coarse_dists, efSearch,
                       do_pruning, heap_order, per=1):
        q = _np(queries, np.float32)
        q = q.reshape(-1, self.d or q.shape[-1])
        nq = q.shape[0]
        cid = None if coarse_ids is None else _np(coarse_ids, np.uint32).reshape(nq, nprobe)
        cd = None if coarse_dists is None else _np(coarse_dists, np.float32).reshape(nq, nprobe)
        qs = None if query_slots is None else _np(query_slots, pick_dtype).reshape(nq * per)
        dist = np.empty((nq, k), np.float32)
        lab = np.empty((nq, k), np.int64)
        p = self._params(nprobe, max_codes, efSearch, do_pruning, heap_order)
        _check(fn(self._h, nq, k, _ptr(q), _ptr(cid), _ptr(cd), C.byref(p), _ptr(qs), _ptr(dist), _ptr(lab)))
        return dist, lab

    def search_slots_dev(self, nq, k, d_queries, d_query_slots, d_distances, d_labels, nprobe, max_codes,
                         d_coarse_ids=None, d_coarse_dists=None, efSearch=0, do_pruning=False, d_out_keys=None,
                         heap_order=False):
        """search_dev() with a filter slot per query (d_query_slots: [nq] bytes in device memory, not checked on the host:
        a byte that names no installed slot passes nothing)."""
        p = self._params(nprobe, max_codes, efSearch, do_pruning, heap_order)
        _check(lib().ivfhnsw_gpu_search_slots_dev(self._h, nq, k, _devptr(d_queries), _devptr(d_coarse_ids),
                                                  _devptr(d_coarse_dists), C.byref(p), _devptr(d_query_slots),
                                                  _devptr(d_distances), _devptr(d_labels), _devptr(d_out_keys)))

    def search_tags_dev(self, nq, k, d_queries, d_query_tags, d_distances, d_labels, nprobe, max_codes,
                        d_coarse_ids=None, d_coarse_dists=None, efSearch=0, do_pruning=False, d_out_keys=None,
                        heap_order=False):
        """search_dev() with a row tag per query (d_query_tags: [nq] uint16 in device memory, not read back)."""
        p = self._params(nprobe, max_codes, efSearch, do_pruning, heap_order)
        _check(lib().ivfhnsw_gpu_search_tags_dev(self._h, nq, k, _devptr(d_queries), _devptr(d_coarse_ids),
                                                 _devptr(d_coarse_dists), C.byref(p), _devptr(d_query_tags),
                                                 _devptr(d_distances), _devptr(d_labels), _devptr(d_out_keys)))

    def search_values_dev(self, nq, k, d_queries, d_query_ranges, d_distances, d_labels, nprobe, max_codes,
                          d_coarse_ids=None, d_coarse_dists=None, efSearch=0, do_pruning=False, d_out_keys=None,
                          heap_order=False):
        """search_dev() with a value interval per query (d_query_ranges: [nq, 2] uint32 in device memory, 8-byte aligned,
        not read back)."""
        p = self._params(nprobe, max_codes, efSearch, do_pruning, heap_order)
        _check(lib().ivfhnsw_gpu_search_values_dev(self._h, nq, k, _devptr(d_queries), _devptr(d_coarse_ids),
                                                   _devptr(d_coarse_dists), C.byref(p), _devptr(d_query_ranges),
                                                   _devptr(d_distances), _devptr(d_labels), _devptr(d_out_keys)))

    def search_tags_values_dev(self, nq, k, d_queries, d_query_tags, d_query_ranges, d_distances, d_labels, nprobe, max_codes,
                               d_coarse_ids=None, d_coarse_dists=None, efSearch=0, do_pruning=False, d_out_keys=None,
                               heap_order=False):
        """search_dev() with a row tag AND a value interval per query (d_query_tags: [nq] uint16, d_query_ranges: [nq, 2]
        uint32 8-byte aligned, both in device memory, not read back); either None gives the other's call."""
        p = self._params(nprobe, max_codes, efSearch, do_pruning, heap_order)
        _check(lib().ivfhnsw_gpu_search_tags_values_dev(self._h, nq, k, _devptr(d_queries), _devptr(d_coarse_ids),
                                                        _devptr(d_coarse_dists), C.byref(p), _devptr(d_query_tags),
                                                        _devptr(d_query_ranges), _devptr(d_distances), _devptr(d_labels),
                                                        _devptr(d_out_keys)))

    # ---- reconstruction of stored vectors (ivfhnsw_gpu_reconstruct*) ---------------------------------
    def locate(self, labels):
        """(rows int64 [n], counts uint32 [n]): the lowest resident row bearing each label (-1 = none) and how many rows
        bear it.  Resident row r = position r of download_ivf()'s ids / codes / norm_codes."""
        lab = _np(labels, np.uint32).ravel()
        rows = np.empty(lab.size, np.int64)
        counts = np.empty(lab.size, np.uint32)
        _check(lib().ivfhnsw_gpu_locate(self._h, lab.size, _ptr(lab) if lab.size else None, _ptr(rows), _ptr(counts)))
        return rows, counts

    def locate_dev(self, n, d_labels, d_rows, d_counts=None):
        """The same on device buffers (torch CUDA tensors or raw addresses); returns with the stream drained."""
        _check(lib().ivfhnsw_gpu_locate_dev(self._h, n, _devptr(d_labels), _devptr(d_rows), _devptr(d_counts)))

    def reconstruct_rows(self, rows, space=RECON_ORIGINAL):
        """float32 [n, d]: the stored vectors of the resident rows (-1 = an empty slot: NaN 0x7fc00000)."""
        r = _np(rows, np.int64).ravel()
        out = np.empty((r.size, self.d), np.float32)
        _check(lib().ivfhnsw_gpu_reconstruct_rows(self._h, r.size, _ptr(r) if r.size else None, space, _ptr(out)))
        return out

    def reconstruct_rows_dev(self, n, d_rows, d_out, space=RECON_ORIGINAL):
        """The same on device buffers, asynchronous on the handle's stream; a row outside [0, n_local) is an empty slot."""
        _check(lib().ivfhnsw_gpu_reconstruct_rows_dev(self._h, n, _devptr(d_rows), space, _devptr(d_out)))

    def reconstruct_list(self, c, space=RECON_ORIGINAL):
        """The vectors of list c, rows offsets[c] .. offsets[c + 1] (faiss reconstruct_n over one list)."""
        off = np.empty(self.nc + 1, np.uint64)
        _check(lib().ivfhnsw_gpu_download_ivf(self._h, _ptr(off), None, None, None))
        return self.reconstruct_rows(np.arange(int(off[c]), int(off[c + 1]), dtype=np.int64), space)

    def reconstruct(self, labels, space=RECON_ORIGINAL):
        """(float32 [n, d], n_missing): the vector stored for each label (its lowest row); a label no row bears gives an
        empty slot and counts in n_missing (faiss reconstruct by id)."""
        lab = _np(labels, np.uint32).ravel()
        out = np.empty((lab.size, self.d), np.float32)
        miss = C.c_uint64(0)
        _check(lib().ivfhnsw_gpu_reconstruct(self._h, lab.size, _ptr(lab) if lab.size else None, space, _ptr(out),
                                             C.byref(miss)))
        return out, int(miss.value)

    def reconstruct_dev(self, n, d_labels, d_out, space=RECON_ORIGINAL, count_missing=True):
        """The same on device buffers; returns n_missing (None, and no wait for the stream, with count_missing=False)."""
        miss = C.c_uint64(0)
        _check(lib().ivfhnsw_gpu_reconstruct_dev(self._h, n, _devptr(d_labels), space, _devptr(d_out),
                                                 C.byref(miss) if count_missing else None))
        return int(miss.value) if count_missing else None

    def search_reconstruct(self, queries, k, nprobe, max_codes, coarse_ids=None, coarse_dists=None, efSearch=0,
                           do_pruning=False, heap_order=False, space=RECON_ORIGINAL):
        """search() plus, for every result, the resident row it came from and that row's vector (faiss
        search_and_reconstruct): (distances [nq, k], labels [nq, k], rows int64 [nq, k], recons float32 [nq, k, d])."""
        q = _np(queries, np.float32)
        q = q.reshape(-1, self.d or q.shape[-1])
        nq = q.shape[0]
        cid = None if coarse_ids is None else _np(coarse_ids, np.uint32).reshape(nq, nprobe)
        cd = None if coarse_dists is None else _np(coarse_dists, np.float32).reshape(nq, nprobe)
        dist = np.empty((nq, k), np.float32)
        lab = np.empty((nq, k), np.int64)
        rows = np.empty((nq, k), np.int64)
        rec = np.empty((nq, k, q.shape[1]), np.float32)
        p = self._params(nprobe, max_codes, efSearch, do_pruning, heap_order)
        _check(lib().ivfhnsw_gpu_search_reconstruct(self._h, nq, k, _ptr(q), _ptr(cid), _ptr(cd), C.byref(p), space,
                                                    _ptr(dist), _ptr(lab), _ptr(rows), _ptr(rec)))
        return dist, lab, rows, rec

    def search_reconstruct_dev(self, nq, k, d_queries, d_distances, d_labels, d_recons, nprobe, max_codes, d_rows=None,
                               d_coarse_ids=None, d_coarse_dists=None, efSearch=0, do_pruning=False, heap_order=False,
                               space=RECON_ORIGINAL):
        """The same on device buffers, asynchronous on the handle's stream."""
        p = self._params(nprobe, max_codes, efSearch, do_pruning, heap_order)
        _check(lib().ivfhnsw_gpu_search_reconstruct_dev(self._h, nq, k, _devptr(d_queries), _devptr(d_coarse_ids),
                                                        _devptr(d_coarse_dists), C.byref(p), space, _devptr(d_distances),
                                                        _devptr(d_labels), _devptr(d_rows), _devptr(d_recons)))

    # ---- range search (ivfhnsw_gpu_range_search) ---------------------------------------------------
    def range_search(self, queries, radius, nprobe, max_codes, efSearch=0, do_pruning=False, coarse_ids=None,
                     coarse_dists=None):
        """Every code the k-search of the same arguments would score with dist < radius (strict), per query in scan
        order: (lims u64 [nq + 1], distances f32 [total], labels i64 [total]); query q owns [lims[q], lims[q + 1])."""
        q = _np(queries, np.float32)
        q = q.reshape(-1, self.d or q.shape[-1])
        nq = q.shape[0]
        cid = None if coarse_ids is None else _np(coarse_ids, np.uint32).reshape(nq, nprobe)
        cd = None if coarse_dists is None else _np(coarse_dists, np.float32).reshape(nq, nprobe)
        lims = np.zeros(nq + 1, np.uint64)
        total = C.c_uint64(0)
        p = self._params(nprobe, max_codes, efSearch, do_pruning)
        _check(lib().ivfhnsw_gpu_range_search(self._h, nq, _ptr(q) if nq else None, _ptr(cid), _ptr(cd), C.byref(p),
                                              C.c_float(radius), _ptr(lims), C.byref(total)))
        dist, lab = self.range_results(0, int(total.value))
        return lims, dist, lab

    def range_search_dev(self, nq, d_queries, radius, d_lims, nprobe, max_codes, efSearch=0, do_pruning=False,
                         d_coarse_ids=None, d_coarse_dists=None):
        """The same on device buffers (d_lims: [nq + 1] 64-bit words); returns when the results are complete, with their
        number.  They stay in the handle's memory: range_results_dev() / range_results()."""
        total = C.c_uint64(0)
        p = self._params(nprobe, max_codes, efSearch, do_pruning)
        _check(lib().ivfhnsw_gpu_range_search_dev(self._h, nq, _devptr(d_queries), _devptr(d_coarse_ids),
                                                  _devptr(d_coarse_dists), C.byref(p), C.c_float(radius), _devptr(d_lims),
                                                  C.byref(total)))
        return int(total.value)

    def range_search_slots(self, queries, radius, query_slots, nprobe, max_codes, efSearch=0, do_pruning=False,
                           coarse_ids=None, coarse_dists=None):
        """range_search() with a filter slot per query (query_slots as search_slots takes them)."""
        return self._range_search_picked(lib().ivfhnsw_gpu_range_search_slots, np.uint8, queries, radius, query_slots, nprobe,
                                         max_codes, efSearch, do_pruning, coarse_ids, coarse_dists)

    def range_search_tags(self, queries, radius, query_tags, nprobe, max_codes, efSearch=0, do_pruning=False,
                          coarse_ids=None, coarse_dists=None):
        """range_search() with a row tag per query (query_tags as search_tags takes them)."""
        return self._range_search_picked(lib().ivfhnsw_gpu_range_search_tags, np.uint16, queries, radius, query_tags, nprobe,
                                         max_codes, efSearch, do_pruning, coarse_ids, coarse_dists)

    def range_search_values(self, queries, radius, query_ranges, nprobe, max_codes, efSearch=0, do_pruning=False,
                            coarse_ids=None, coarse_dists=None):
        """range_search() with a value interval per query (query_ranges as search_values takes them)."""
        return self._range_search_picked(lib().ivfhnsw_gpu_range_search_values, np.uint32, queries, radius, query_ranges, nprobe,
                                         max_codes, efSearch, do_pruning, coarse_ids, coarse_dists, per=2)

    def range_search_tags_values(self, queries, radius, query_tags, query_ranges, nprobe, max_codes, efSearch=0,
                                 do_pruning=False, coarse_ids=None, coarse_dists=None):
        """range_search() with a row tag AND a value interval per query (as search_tags_values takes them)."""
        q = _np(queries, np.float32)
        q = q.reshape(-1, self.d or q.shape[-1])
        nq = q.shape[0]
        cid = None if coarse_ids is None else _np(coarse_ids, np.uint32).reshape(nq, nprobe)
        cd = None if coarse_dists is None else _np(coarse_dists, np.float32).reshape(nq, nprobe)
        qt = None if query_tags is None else _np(query_tags, np.uint16).reshape(nq)
        qr = None if query_ranges is None else _np(query_ranges, np.uint32).reshape(nq * 2)
        lims = np.zeros(nq + 1, np.uint64)
        total = C.c_uint64(0)
        p = self._params(nprobe, max_codes, efSearch, do_pruning)
        _check(lib().ivfhnsw_gpu_range_search_tags_values(self._h, nq, _ptr(q) if nq else None, _ptr(cid), _ptr(cd), C.byref(p),
                                                          _ptr(qt), _ptr(qr), C.c_float(radius), _ptr(lims), C.byref(total)))
        dist, lab = self.range_results(0, int(total.value))
        return lims, dist, lab

    def _range_search_picked(self, fn, pick_dtype, queries, radius, query_slots, nprobe, max_codes, efSearch, do_pruning,
                             coarse_ids, coarse_dists, per=1):
        q = _np(queries, np.float32)
        q = q.reshape(-1, self.d or q.shape[-1])
        nq = q.shape[0]
        cid = None if coarse_ids is None else _np(coarse_ids, np.uint32).reshape(nq, nprobe)
        cd = None if coarse_dists is None else _np(coarse_dists, np.float32).reshape(nq, nprobe)
        qs = None if query_slots is None else _np(query_slots, pick_dtype).reshape(nq * per)
        lims = np.zeros(nq + 1, np.uint64)
        total = C.c_uint64(0)
        p = self._params(nprobe, max_codes, efSearch, do_pruning)
        _check(fn(self._h, nq, _ptr(q) if nq else None, _ptr(cid), _ptr(cd), C.byref(p), _ptr(qs), C.c_float(radius),
                  _ptr(lims), C.byref(total)))
        dist, lab = self.range_results(0, int(total.value))
        return lims, dist, lab

    def range_search_slots_dev(self, nq, d_queries, radius, d_query_slots, d_lims, nprobe, max_codes, efSearch=0,
                               do_pruning=False, d_coarse_ids=None, d_coarse_dists=None):
        """range_search_dev() with a filter slot per query (d_query_slots in device memory)."""
        total = C.c_uint64(0)
        p = self._params(nprobe, max_codes, efSearch, do_pruning)
        _check(lib().ivfhnsw_gpu_range_search_slots_dev(self._h, nq, _devptr(d_queries), _devptr(d_coarse_ids),
                                                        _devptr(d_coarse_dists), C.byref(p), _devptr(d_query_slots),
                                                        C.c_float(radius), _devptr(d_lims), C.byref(total)))
        return int(total.value)

    def range_search_tags_dev(self, nq, d_queries, radius, d_query_tags, d_lims, nprobe, max_codes, efSearch=0,
                              do_pruning=False, d_coarse_ids=None, d_coarse_dists=None):
        """range_search_dev() with a row tag per query (d_query_tags in device memory)."""
        total = C.c_uint64(0)
        p = self._params(nprobe, max_codes, efSearch, do_pruning)
        _check(lib().ivfhnsw_gpu_range_search_tags_dev(self._h, nq, _devptr(d_queries), _devptr(d_coarse_ids),
                                                       _devptr(d_coarse_dists), C.byref(p), _devptr(d_query_tags),
                                                       C.c_float(radius), _devptr(d_lims), C.byref(total)))
        return int(total.value)

    def range_search_values_dev(self, nq, d_queries, radius, d_query_ranges, d_lims, nprobe, max_codes, efSearch=0,
                                do_pruning=False, d_coarse_ids=None, d_coarse_dists=None):
        """range_search_dev() with a value interval per query (d_query_ranges in device memory)."""
        total = C.c_uint64(0)
        p = self._params(nprobe, max_codes, efSearch, do_pruning)
        _check(lib().ivfhnsw_gpu_range_search_values_dev(self._h, nq, _devptr(d_queries), _devptr(d_coarse_ids),
                                                         _devptr(d_coarse_dists), C.byref(p), _devptr(d_query_ranges),
                                                         C.c_float(radius), _devptr(d_lims), C.byref(total)))
        return int(total.value)

    def range_search_tags_values_dev(self, nq, d_queries, radius, d_query_tags, d_query_ranges, d_lims, nprobe, max_codes,
                                     efSearch=0, do_pruning=False, d_coarse_ids=None, d_coarse_dists=None):
        """range_search_dev() with a row tag AND a value interval per query (both arrays in device memory)."""
        total = C.c_uint64(0)
        p = self._params(nprobe, max_codes, efSearch, do_pruning)
        _check(lib().ivfhnsw_gpu_range_search_tags_values_dev(self._h, nq, _devptr(d_queries), _devptr(d_coarse_ids),
                                                              _devptr(d_coarse_dists), C.byref(p), _devptr(d_query_tags),
                                                              _devptr(d_query_ranges), C.c_float(radius), _devptr(d_lims),
                                                              C.byref(total)))
        return int(total.value)

    def range_results(self, first, count):
        """Entries [first, first + count) of the last range search's results: (distances f32, labels i64)."""
        dist = np.empty(count, np.float32)
        lab = np.empty(count, np.int64)
        _check(lib().ivfhnsw_gpu_range_results(self._h, first, count, _ptr(dist), _ptr(lab)))
        return dist, lab

    def range_results_dev(self):
        """(distance pointer, label pointer, total) of the last range search's results in the handle's memory (raw device
        addresses, 0 when the total is 0), valid until this handle's next range search, upload_ivf or close."""
        pd, pl, total = C.c_void_p(), C.c_void_p(), C.c_uint64(0)
        _check(lib().ivfhnsw_gpu_range_results_dev(self._h, C.byref(pd), C.byref(pl), C.byref(total)))
        return pd.value or 0, pl.value or 0, int(total.value)

    def resolve_keys_dev(self, nq, k, d_keys, d_distances, d_labels):
        _check(lib().ivfhnsw_gpu_resolve_keys_dev(self._h, nq, k, _devptr(d_keys), _devptr(d_distances),
                                                  _devptr(d_labels)))

    def last_stream_dev(self, nq, len_cap=0, d_keys=None, d_len=None):
        """Copy out the candidate streams the last search_dev (k > 1, heap_order, out_keys) left: lengths into d_len
        ([nq] int32), the first len_cap keys of each into d_keys ([nq, len_cap] int64).  Returns the stream capacity."""
        cap = C.c_uint32()
        _check(lib().ivfhnsw_gpu_last_stream_dev(self._h, nq, len_cap, _devptr(d_keys), _devptr(d_len), C.byref(cap)))
        return cap.value

    def replay_stream_dev(self, nq, k, d_stream, d_len, cap, d_out_keys):
        _check(lib().ivfhnsw_gpu_replay_stream_dev(self._h, nq, k, _devptr(d_stream), _devptr(d_len), cap,
                                                   _devptr(d_out_keys)))

    def rotate_dev(self, nq, d_queries, d_out):
        """opq_matrix->apply on device buffers (a copy when the index has no OPQ matrix)."""
        _check(lib().ivfhnsw_gpu_rotate_dev(self._h, nq, _devptr(d_queries), _devptr(d_out)))

    def coarse_dev(self, nq, d_queries, nprobe, efSearch, d_coarse_ids, d_coarse_dists):
        _check(lib().ivfhnsw_gpu_coarse_dev(self._h, nq, _devptr(d_queries), nprobe, efSearch,
                                            _devptr(d_coarse_ids), _devptr(d_coarse_dists)))

    def coarse(self, queries, k, efSearch):
        """Host arrays: the HNSW walk alone (k = 1: IndexIVF_HNSW::assign)."""
        q = _np(queries, np.float32)
        q = q.reshape(-1, q.shape[-1])
        ids = np.empty((q.shape[0], k), np.uint32)
        dist = np.empty((q.shape[0], k), np.float32)
        _check(lib().ivfhnsw_gpu_coarse(self._h, q.shape[0], _ptr(q), k, efSearch, _ptr(ids), _ptr(dist)))
        return ids, dist

    # ---- construction side ------------------------------------------------------------------------
    def upload_codebooks(self, d, code_size, pq_centroids, norm_table, opq_A=None):
        pq = _np(pq_centroids, np.float32)
        nt = _np(norm_table, np.float32)
        assert pq.size == 256 * d and nt.size == 256
        A = None if opq_A is None else _np(opq_A, np.float32)
        _check(lib().ivfhnsw_gpu_upload_codebooks(self._h, d, code_size, _ptr(pq), _ptr(nt), _ptr(A)))
        self._enc_M = code_size

    def encode(self, x, precomputed_idx=None, efSearch=0):
        """IndexIVF_HNSW::add_batch up to the append loop (IndexIVF_HNSW.cpp:75-121): (idx, codes, norm_codes)."""
        x = _np(x, np.float32)
        x = x.reshape(-1, x.shape[-1])
        n = x.shape[0]
        pidx = None if precomputed_idx is None else _np(precomputed_idx, np.uint32)
        idx = np.empty(n, np.uint32)
        codes = np.empty((n, self._enc_M), np.uint8)
        ncodes = np.empty(n, np.uint8)
        _check(lib().ivfhnsw_gpu_encode(self._h, n, _ptr(x), _ptr(pidx), efSearch, _ptr(idx), _ptr(codes), _ptr(ncodes)))
        return idx, codes, ncodes

    def encode_groups(self, nsubc, centroid_idx, offsets, x, efSearch, alphas_in=None):
        """IndexIVF_HNSW_Grouping::add_group for many groups (Grouping.cpp:43-125):
        (nn_centroid_idxs [G, nsubc], alphas [G], subcentroid_idxs [n], codes [n, M], norm_codes [n])."""
        cidx = _np(centroid_idx, np.uint32)
        off = _np(offsets, np.uint64)
        G = cidx.shape[0]
        x = _np(x, np.float32)
        x = x.reshape(-1, x.shape[-1]) if x.size else x.reshape(0, 1)
        n = int(off[-1])
        nn = np.empty((G, nsubc), np.uint32)
        alphas = np.zeros(G, np.float32) if alphas_in is None else _np(alphas_in, np.float32).copy()
        sub = np.empty(n, np.uint32)
        codes = np.empty((n, self._enc_M), np.uint8)
        ncodes = np.empty(n, np.uint8)
        _check(lib().ivfhnsw_gpu_encode_groups(self._h, G, nsubc, _ptr(cidx), _ptr(off), _ptr(x), efSearch, _ptr(nn),
                                               _ptr(alphas), _ptr(sub), _ptr(codes), _ptr(ncodes)))
        return nn, alphas, sub, codes, ncodes

    def pq_train(self, x, M, centroids, niter=1):
        """niter Lloyd iterations of ProductQuantizer::train on the device: (centroids [M, 256, d/M], assign [n, M])."""
        x = _np(x, np.float32)
        n, d = x.shape
        c = _np(centroids, np.float32).copy().reshape(M, 256, d // M)
        a = np.empty((n, M), np.uint8)
        _check(lib().ivfhnsw_gpu_pq_train(self._h, n, d, M, _ptr(x), niter, _ptr(c), _ptr(a)))
        return c, a

    def xty(self, X, Y):
        """X^T Y of OPQ's Procrustes step on the matrix cores ([n, d] each -> [d, d])."""
        X = _np(X, np.float32)
        Y = _np(Y, np.float32)
        n, d = X.shape
        out = np.empty((d, d), np.float32)
        _check(lib().ivfhnsw_gpu_xty(self._h, n, d, _ptr(X), _ptr(Y), _ptr(out)))
        return out

    def kmeans(self, x, centroids, niter):
        """niter exact Lloyd iterations of the coarse centroids (ivfhnsw_gpu_kmeans): x [n, d], seeds [nc, d] ->
        (centroids f32 [nc, d], assign u32 [n] of the last iteration, obj f64 [niter])."""
        x = _np(x, np.float32)
        n, d = x.shape
        c = _np(centroids, np.float32).reshape(-1, d).copy()
        a = np.zeros(n, np.uint32)
        obj = np.zeros(niter, np.float64)
        _check(lib().ivfhnsw_gpu_kmeans(self._h, n, d, c.shape[0], _ptr(x), niter, _ptr(c), _ptr(a), _ptr(obj)))
        return c, a, obj

    def kmeans_dev(self, n, d, nc, d_x, niter, d_centroids, d_assign=None):
        """The same on device buffers (torch CUDA tensors; d_centroids updated in place, d_assign [n] u32/i32 or None);
        returns obj f64 [niter] (host)."""
        obj = np.zeros(niter, np.float64)
        _check(lib().ivfhnsw_gpu_kmeans_dev(self._h, n, d, nc, _devptr(d_x), niter, _devptr(d_centroids),
                                            _devptr(d_assign), _ptr(obj)))
        return obj

    KNN_ALL, KNN_NOT_SELF, KNN_EARLIER = 0, 1, 2

    def knn(self, base, k, queries=None, mode=None):
        """Exact k nearest base rows of every query row (ivfhnsw_gpu_knn; queries=None: of every base row, by default
        itself left out; mode KNN_EARLIER: only rows before it): (ids u32 [nq, k], dists f32 [nq, k]) ascending by
        (dist, id)."""
        if mode is None:
            mode = self.KNN_NOT_SELF if queries is None else self.KNN_ALL
        x = _np(base, np.float32)
        nx, d = x.shape
        q = None if queries is None else _np(queries, np.float32).reshape(-1, d)
        nq = nx if q is None else q.shape[0]
        ids = np.empty((nq, k), np.uint32)
        dist = np.empty((nq, k), np.float32)
        _check(lib().ivfhnsw_gpu_knn(self._h, nq, nx, d, _ptr(q), _ptr(x), k, mode, _ptr(ids), _ptr(dist)))
        return ids, dist

    def knn_dev(self, nq, nx, d, d_queries, d_base, k, d_ids, d_dists=None, exclude_self=False, mode=None):
        """The same on device buffers (torch CUDA tensors), asynchronous on the handle's stream."""
        if mode is None:
            mode = self.KNN_NOT_SELF if exclude_self else self.KNN_ALL
        _check(lib().ivfhnsw_gpu_knn_dev(self._h, nq, nx, d, _devptr(d_queries), _devptr(d_base), k, mode,
                                         _devptr(d_ids), _devptr(d_dists)))

    def build_graph(self, vectors, M=16, maxM=32, ncand=64):
        """hnswlib's addPoint loop for all nodes at once, candidates = the exact ncand nearest earlier nodes
        (ivfhnsw_gpu_build_graph): (counts u8 [n], links u32 [n, maxM])."""
        v = _np(vectors, np.float32)
        n, d = v.shape
        counts = np.zeros(n, np.uint8)
        links = np.zeros((n, maxM), np.uint32)
        _check(lib().ivfhnsw_gpu_build_graph(self._h, n, d, _ptr(v), M, maxM, ncand, _ptr(counts), _ptr(links)))
        return counts, links

    def build_graph_dev(self, n, d, d_vectors, M, maxM, ncand, d_counts, d_links):
        """The same on device buffers (torch CUDA tensors: d_vectors f32 [n, d], d_counts u8 [n], d_links u32/i32
        [n, maxM]), asynchronous on the handle's stream."""
        _check(lib().ivfhnsw_gpu_build_graph_dev(self._h, n, d, _devptr(d_vectors), M, maxM, ncand, _devptr(d_counts),
                                                 _devptr(d_links)))

    def last_graph_longest_reverse(self):
        """The longest reverse list (later nodes that chose one node) of the last build_graph[_dev]."""
        v = C.c_uint64(0)
        _check(lib().ivfhnsw_gpu_last_graph_longest_reverse(self._h, C.byref(v)))
        return v.value

    def set_option(self, key, value):
        """Library options (ivfhnsw_gpu_set_option), e.g. ("scan_pipe", 0)."""
        _check(lib().ivfhnsw_gpu_set_option(self._h, key.encode(), int(value)))

    def sync(self):
        _check(lib().ivfhnsw_gpu_sync(self._h))

    def set_stream(self, stream_ptr):
        _check(lib().ivfhnsw_gpu_set_stream(self._h, C.c_void_p(stream_ptr)))

    # ---- exact re-rank (IndexIVF_HNSW_Grouping::searchDisk) --------------------------------------------------------
    def upload_base(self, rows_u8, n=None, first=0, row_stride=None):
        """Rows [first, first + count) of the uint8 base store (ivfhnsw_gpu_upload_base).  rows_u8: [count, d] uint8 whose
        rows may lie row_stride bytes apart (default: its own row stride; raw[:, 4:] of a [count, d + 4] .bvecs image
        is taken as it is).  n: rows of the whole store (default first + count); first == 0 (re)allocates it."""
        a = np.asarray(rows_u8)
        assert a.dtype == np.uint8 and a.ndim == 2, "rows_u8: a 2-D uint8 array [count, d]"
        count, d = a.shape
        stride = a.strides[0] if row_stride is None else row_stride
        assert count == 0 or (a.strides[1] == 1 and (count == 1 or a.strides[0] == stride)), \
            "rows must be contiguous inside a row and row_stride apart"
        n = first + count if n is None else n
        _check(lib().ivfhnsw_gpu_upload_base(self._h, n, d, first, count, C.c_void_p(a.ctypes.data) if count else None,
                                             max(stride, d)))
        self.base_n, self.base_d = n, d

    def upload_base_dev(self, n, d, first, count, d_rows, row_stride=None):
        """The same from HBM (a torch CUDA uint8 tensor or a device address); synchronous."""
        _check(lib().ivfhnsw_gpu_upload_base_dev(self._h, n, d, first, count, _devptr(d_rows),
                                                 d if row_stride is None else row_stride))
        self.base_n, self.base_d = n, d

    def upload_base_bvecs(self, path, chunk_rows=1 << 20, rows=None):
        """Stream a .bvecs file (records: int32 dim + dim bytes) into the base store in chunks of chunk_rows records
        (rows: only the file's first `rows` records); every record's dim header is checked."""
        n, d = xvecs_shape(path, 1)
        if rows is not None:
            if not 1 <= rows <= n:
                raise ValueError("%s holds %d records, asked for the first %d" % (path, n, rows))
            n = rows
        rec = d + 4
        with open(path, "rb") as f:
            for first in range(0, n, chunk_rows):
                m = min(chunk_rows, n - first)
                raw = np.frombuffer(f.read(m * rec), np.uint8).reshape(m, rec)
                _check_dims(path, raw[:, :4].copy().view(np.int32)[:, 0], d, first)
                self.upload_base(raw[:, 4:], n=n, first=first, row_stride=rec)
        return n, d

    def rerank(self, queries, cand, k):
        """Host arrays: the k best of every query's candidate labels ([nq, kc] int64, -1 = empty) by (exact L2 against
        the base store, label): (distances f32 [nq, k], labels i64 [nq, k])."""
        c = _np(cand, np.int64)
        c = c.reshape(c.shape[0] if c.ndim > 1 else 1, -1)
        nq, kc = c.shape
        q = _np(queries, np.float32).reshape(nq, -1)
        dist = np.empty((nq, k), np.float32)
        lab = np.empty((nq, k), np.int64)
        _check(lib().ivfhnsw_gpu_rerank(self._h, nq, kc, _ptr(q), _ptr(c), k, _ptr(dist), _ptr(lab)))
        return dist, lab

    def rerank_dev(self, nq, kc, d_queries, d_cand, k, d_distances, d_labels):
        """Device buffers (torch CUDA tensors), asynchronous on the handle's stream."""
        _check(lib().ivfhnsw_gpu_rerank_dev(self._h, nq, kc, _devptr(d_queries), _devptr(d_cand), k, _devptr(d_distances),
                                            _devptr(d_labels)))

    def search_rerank(self, queries, k, kc, nprobe, max_codes, efSearch=0, do_pruning=False, coarse_ids=None,
                      coarse_dists=None):
        """searchDisk for a batch: search_dev for kc candidates (ascending, heap_order 0), then rerank_dev on the same
        stream, with no host round trip in between.  Host arrays in and out: (distances [nq, k], labels [nq, k])."""
        import torch
        q = _np(queries, np.float32)
        q = q.reshape(-1, self.d or q.shape[-1])
        nq = q.shape[0]
        dev = torch.device("cuda", self._device)
        tq = torch.from_numpy(q).to(dev)
        tcid = None if coarse_ids is None else torch.from_numpy(_np(coarse_ids, np.uint32).reshape(nq, nprobe).view(np.int32)).to(dev)
        tcd = None if coarse_dists is None else torch.from_numpy(_np(coarse_dists, np.float32).reshape(nq, nprobe)).to(dev)
        cd = torch.empty((nq, kc), dtype=torch.float32, device=dev)
        cl = torch.empty((nq, kc), dtype=torch.int64, device=dev)
        od = torch.empty((nq, k), dtype=torch.float32, device=dev)
        ol = torch.empty((nq, k), dtype=torch.int64, device=dev)
        torch.cuda.synchronize(dev)  # the copies above ran on torch's stream, the library runs on the handle's
        self.search_dev(nq, kc, tq, cd, cl, nprobe, max_codes, d_coarse_ids=tcid, d_coarse_dists=tcd, efSearch=efSearch,
                        do_pruning=do_pruning)
        self.rerank_dev(nq, kc, tq, cl, k, od, ol)
        self.sync()
        return od.cpu().numpy(), ol.cpu().numpy()

    # ---- exact brute-force search of the base store (ground truth) -------------------------------------------------
    def exact_search(self, queries_u8, k):
        """The k rows of the base store nearest to every query by exact integer squared L2 (ivfhnsw_gpu_exact_search):
        queries_u8 [nq, d] uint8 whose rows may lie a row stride apart (raw[:, 4:] of a .bvecs image is taken as it is).
        Returns (distances f32 [nq, k], labels i64 [nq, k]) ascending by (distance, label), padded FLT_MAX / -1."""
        a = np.asarray(queries_u8)
        assert a.dtype == np.uint8 and a.ndim == 2, "queries_u8: a 2-D uint8 array [nq, d]"
        nq, d = a.shape
        assert nq == 0 or (a.strides[1] == 1 and (nq == 1 or a.strides[0] >= d)), \
            "queries must be contiguous inside a row and a fixed stride apart"
        stride = a.strides[0] if nq > 1 else d
        dist = np.empty((nq, k), np.float32)
        lab = np.empty((nq, k), np.int64)
        _check(lib().ivfhnsw_gpu_exact_search(self._h, nq, C.c_void_p(a.ctypes.data) if nq else None, stride, k, _ptr(dist),
                                              _ptr(lab)))
        return dist, lab

    def exact_search_dev(self, nq, d_queries, row_stride, k, d_distances, d_labels):
        """The same on device buffers (torch CUDA tensors or raw addresses), asynchronous on the handle's stream."""
        _check(lib().ivfhnsw_gpu_exact_search_dev(self._h, nq, _devptr(d_queries), row_stride, k, _devptr(d_distances),
                                                  _devptr(d_labels)))

    # ---- exact range search of the base store (ivfhnsw_gpu_exact_range_search) ----------------------
    def exact_range_search(self, queries_u8, radius):
        """Every row of the base store with float(exact integer squared L2) < radius (strict), per query in ascending
        label: (lims u64 [nq + 1], distances f32 [total], labels i64 [total]); query q owns [lims[q], lims[q + 1]).
        queries_u8 [nq, d] uint8 whose rows may lie a row stride apart, as exact_search takes them."""
        a = np.asarray(queries_u8)
        assert a.dtype == np.uint8 and a.ndim == 2, "queries_u8: a 2-D uint8 array [nq, d]"
        nq, d = a.shape
        assert nq == 0 or (a.strides[1] == 1 and (nq == 1 or a.strides[0] >= d)), \
            "queries must be contiguous inside a row and a fixed stride apart"
        stride = a.strides[0] if nq > 1 else d
        lims = np.zeros(nq + 1, np.uint64)
        total = C.c_uint64(0)
        _check(lib().ivfhnsw_gpu_exact_range_search(self._h, nq, C.c_void_p(a.ctypes.data) if nq else None, stride,
                                                    C.c_float(radius), _ptr(lims), C.byref(total)))
        dist, lab = self.exact_range_results(0, int(total.value))
        return lims, dist, lab

    def exact_range_search_dev(self, nq, d_queries, row_stride, radius, d_lims):
        """The same on device buffers (d_lims: [nq + 1] 64-bit words); returns when the results are complete, with their
        number.  They stay in the handle's memory: exact_range_results_dev() / exact_range_results()."""
        total = C.c_uint64(0)
        _check(lib().ivfhnsw_gpu_exact_range_search_dev(self._h, nq, _devptr(d_queries), row_stride, C.c_float(radius),
                                                        _devptr(d_lims), C.byref(total)))
        return int(total.value)

    def exact_range_results(self, first, count):
        """Entries [first, first + count) of the last exact range search's results: (distances f32, labels i64)."""
        dist = np.empty(count, np.float32)
        lab = np.empty(count, np.int64)
        _check(lib().ivfhnsw_gpu_exact_range_results(self._h, first, count, _ptr(dist), _ptr(lab)))
        return dist, lab

    def exact_range_results_dev(self):
        """(distance pointer, label pointer, total) of the last exact range search's results in the handle's memory (raw
        device addresses, 0 when the total is 0), valid until this handle's next exact range search or close."""
        pd, pl, total = C.c_void_p(), C.c_void_p(), C.c_uint64(0)
        _check(lib().ivfhnsw_gpu_exact_range_results_dev(self._h, C.byref(pd), C.byref(pl), C.byref(total)))
        return pd.value or 0, pl.value or 0, int(total.value)

    # ---- base filter of the exact calls (ivfhnsw_gpu_set_base_filter) ------------------------------
    def set_base_filter(self, labels, deny=False):
        """exact_search and exact_range_search consider only the rows of the base store whose row number is in `labels`
        (deny=True: is not in them); replaces an earlier base filter.  Independent of set_filter."""
        lab = _np(labels, np.uint32).ravel()
        _check(lib().ivfhnsw_gpu_set_base_filter(self._h, lab.size, _ptr(lab) if lab.size else None,
                                                 FILTER_DENY if deny else FILTER_ALLOW))

    def set_base_filter_dev(self, n, d_labels, deny=False):
        """The same on a device buffer (torch CUDA tensor or raw address)."""
        _check(lib().ivfhnsw_gpu_set_base_filter_dev(self._h, n, _devptr(d_labels), FILTER_DENY if deny else FILTER_ALLOW))

    def clear_base_filter(self):
        _check(lib().ivfhnsw_gpu_clear_base_filter(self._h))

    def base_filter_info(self):
        """(mode or -1, rows_passing, rows_total) of the base store."""
        m, a, b = C.c_int(-1), C.c_uint64(0), C.c_uint64(0)
        _check(lib().ivfhnsw_gpu_base_filter_info(self._h, C.byref(m), C.byref(a), C.byref(b)))
        return int(m.value), int(a.value), int(b.value)

    # ---- base filter slots: a base filter per query (ivfhnsw_gpu_set_base_filter_slot) --------------
    def set_base_filter_slot(self, slot, labels, deny=False):
        """Base filter slot `slot` (0..FILTER_SLOTS-1) holds the row numbers `labels`, allow or deny as set_base_filter;
        replaces the slot's earlier set.  The exact _slots calls name a slot per query."""
        lab = _np(labels, np.uint32).ravel()
        _check(lib().ivfhnsw_gpu_set_base_filter_slot(self._h, slot, lab.size, _ptr(lab) if lab.size else None,
                                                      FILTER_DENY if deny else FILTER_ALLOW))

    def set_base_filter_slot_dev(self, slot, n, d_labels, deny=False):
        """The same on a device buffer (torch CUDA tensor or raw address)."""
        _check(lib().ivfhnsw_gpu_set_base_filter_slot_dev(self._h, slot, n, _devptr(d_labels),
                                                          FILTER_DENY if deny else FILTER_ALLOW))

    def clear_base_filter_slot(self, slot=None):
        """The slot passes nothing afterwards; None: every slot."""
        _check(lib().ivfhnsw_gpu_clear_base_filter_slot(self._h, -1 if slot is None else slot))

    def base_filter_slot_info(self, slot):
        """(mode or -1, rows_passing, rows_total) of one base filter slot."""
        m, a, b = C.c_int(-1), C.c_uint64(0), C.c_uint64(0)
        _check(lib().ivfhnsw_gpu_base_filter_slot_info(self._h, slot, C.byref(m), C.byref(a), C.byref(b)))
        return int(m.value), int(a.value), int(b.value)

    @staticmethod
    def _exact_queries(queries_u8):
        a = np.asarray(queries_u8)
        assert a.dtype == np.uint8 and a.ndim == 2, "queries_u8: a 2-D uint8 array [nq, d]"
        nq, d = a.shape
        assert nq == 0 or (a.strides[1] == 1 and (nq == 1 or a.strides[0] >= d)), \
            "queries must be contiguous inside a row and a fixed stride apart"
        return a, nq, (a.strides[0] if nq > 1 else d)

    def exact_search_slots(self, queries_u8, k, query_slots):
        """exact_search() with a base filter slot per query: query_slots [nq] bytes, each a slot or SLOT_NONE (no
        filter); None is exact_search() itself (ivfhnsw_gpu_exact_search_slots)."""
        a, nq, stride = self._exact_queries(queries_u8)
        qs = None if query_slots is None else _np(query_slots, np.uint8).reshape(nq)
        dist = np.empty((nq, k), np.float32)
        lab = np.empty((nq, k), np.int64)
        _check(lib().ivfhnsw_gpu_exact_search_slots(self._h, nq, C.c_void_p(a.ctypes.data) if nq else None, stride, k,
                                                    _ptr(qs), _ptr(dist), _ptr(lab)))
        return dist, lab

    def exact_search_slots_dev(self, nq, d_queries, row_stride, k, d_query_slots, d_distances, d_labels):
        """The same on device buffers (d_query_slots: [nq] bytes in device memory, not checked on the host: a byte that
        names no installed slot passes nothing), asynchronous on the handle's stream."""
        _check(lib().ivfhnsw_gpu_exact_search_slots_dev(self._h, nq, _devptr(d_queries), row_stride, k,
                                                        _devptr(d_query_slots), _devptr(d_distances), _devptr(d_labels)))

    def exact_range_search_slots(self, queries_u8, radius, query_slots):
        """exact_range_search() with a base filter slot per query; lims in the caller's query order."""
        a, nq, stride = self._exact_queries(queries_u8)
        qs = None if query_slots is None else _np(query_slots, np.uint8).reshape(nq)
        lims = np.zeros(nq + 1, np.uint64)
        total = C.c_uint64(0)
        _check(lib().ivfhnsw_gpu_exact_range_search_slots(self._h, nq, C.c_void_p(a.ctypes.data) if nq else None, stride,
                                                          _ptr(qs), C.c_float(radius), _ptr(lims), C.byref(total)))
        dist, lab = self.exact_range_results(0, int(total.value))
        return lims, dist, lab

    def exact_range_search_slots_dev(self, nq, d_queries, row_stride, d_query_slots, radius, d_lims):
        """The same on device buffers; returns the number of results, which stay in the handle's memory."""
        total = C.c_uint64(0)
        _check(lib().ivfhnsw_gpu_exact_range_search_slots_dev(self._h, nq, _devptr(d_queries), row_stride,
                                                              _devptr(d_query_slots), C.c_float(radius), _devptr(d_lims),
                                                              C.byref(total)))
        return int(total.value)

    # ---- base tags: a 16-bit tag per store row, a tag per query (ivfhnsw_gpu_set_base_tags) ---------
    def set_base_tags(self, rows, tags):
        """The rows of the base store given carry the tags given (uint16; TAG_NONE untags) from now on; every other row
        keeps its tag.  The exact _tags calls name a tag per query."""
        r = _np(rows, np.uint32).ravel()
        tg = _np(tags, np.uint16).ravel()
        if tg.size != r.size:
            raise ValueError("set_base_tags: %d rows, %d tags" % (r.size, tg.size))
        _check(lib().ivfhnsw_gpu_set_base_tags(self._h, r.size, _ptr(r) if r.size else None, _ptr(tg) if tg.size else None))

    def set_base_tags_dev(self, n, d_rows, d_tags):
        """The same on device buffers (torch CUDA tensors or raw addresses)."""
        _check(lib().ivfhnsw_gpu_set_base_tags_dev(self._h, n, _devptr(d_rows), _devptr(d_tags)))

    def clear_base_tags(self):
        """No row of the base store is tagged afterwards."""
        _check(lib().ivfhnsw_gpu_clear_base_tags(self._h))

    def base_tags_info(self):
        """(rows_tagged, rows_total, tags_in_use) of the base store."""
        a, b, c = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        _check(lib().ivfhnsw_gpu_base_tags_info(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return int(a.value), int(b.value), int(c.value)

    def base_tag_rows(self, tag):
        """Rows of the base store that carry `tag`."""
        n = C.c_uint64(0)
        _check(lib().ivfhnsw_gpu_base_tag_rows(self._h, tag, C.byref(n)))
        return int(n.value)

    def exact_search_tags(self, queries_u8, k, query_tags):
        """exact_search() with a tag per query: query_tags [nq] uint16, each a tag or TAG_NONE (no restriction); None is
        exact_search() itself (ivfhnsw_gpu_exact_search_tags)."""
        a, nq, stride = self._exact_queries(queries_u8)
        qt = None if query_tags is None else _np(query_tags, np.uint16).reshape(nq)
        dist = np.empty((nq, k), np.float32)
        lab = np.empty((nq, k), np.int64)
        _check(lib().ivfhnsw_gpu_exact_search_tags(self._h, nq, C.c_void_p(a.ctypes.data) if nq else None, stride, k,
                                                   _ptr(qt), _ptr(dist), _ptr(lab)))
        return dist, lab

    def exact_search_tags_dev(self, nq, d_queries, row_stride, k, d_query_tags, d_distances, d_labels):
        """The same on device buffers (d_query_tags: [nq] uint16 in device memory), asynchronous on the handle's stream."""
        _check(lib().ivfhnsw_gpu_exact_search_tags_dev(self._h, nq, _devptr(d_queries), row_stride, k,
                                                       _devptr(d_query_tags), _devptr(d_distances), _devptr(d_labels)))

    def exact_range_search_tags(self, queries_u8, radius, query_tags):
        """exact_range_search() with a tag per query; lims in the caller's query order."""
        a, nq, stride = self._exact_queries(queries_u8)
        qt = None if query_tags is None else _np(query_tags, np.uint16).reshape(nq)
        lims = np.zeros(nq + 1, np.uint64)
        total = C.c_uint64(0)
        _check(lib().ivfhnsw_gpu_exact_range_search_tags(self._h, nq, C.c_void_p(a.ctypes.data) if nq else None, stride,
                                                         _ptr(qt), C.c_float(radius), _ptr(lims), C.byref(total)))
        dist, lab = self.exact_range_results(0, int(total.value))
        return lims, dist, lab

    def exact_range_search_tags_dev(self, nq, d_queries, row_stride, d_query_tags, radius, d_lims):
        """The same on device buffers; returns the number of results, which stay in the handle's memory."""
        total = C.c_uint64(0)
        _check(lib().ivfhnsw_gpu_exact_range_search_tags_dev(self._h, nq, _devptr(d_queries), row_stride,
                                                             _devptr(d_query_tags), C.c_float(radius), _devptr(d_lims),
                                                             C.byref(total)))
        return int(total.value)

    # ---- base values: a uint32 per store row, an interval per query (ivfhnsw_gpu_set_base_values) ----
    def set_base_values(self, rows, values):
        """The rows of the base store given hold the values given (uint32; VALUE_NONE un-values) from now on; every other
        row keeps its value.  The exact _values calls name an interval per query."""
        r = _np(rows, np.uint32).ravel()
        v = _np(values, np.uint32).ravel()
        if v.size != r.size:
            raise ValueError("set_base_values: %d rows, %d values" % (r.size, v.size))
        _check(lib().ivfhnsw_gpu_set_base_values(self._h, r.size, _ptr(r) if r.size else None, _ptr(v) if v.size else None))

    def set_base_values_dev(self, n, d_rows, d_values):
        """The same on device buffers (torch CUDA tensors or raw addresses)."""
        _check(lib().ivfhnsw_gpu_set_base_values_dev(self._h, n, _devptr(d_rows), _devptr(d_values)))

    def clear_base_values(self):
        """No row of the base store holds a value afterwards."""
        _check(lib().ivfhnsw_gpu_clear_base_values(self._h))

    def base_values_info(self):
        """(rows_valued, rows_total) of the base store."""
        a, b = C.c_uint64(0), C.c_uint64(0)
        _check(lib().ivfhnsw_gpu_base_values_info(self._h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def base_value_rows(self, lo, hi):
        """Rows of the base store whose value lies in [lo, hi] (a valueless row holds VALUE_NONE)."""
        n = C.c_uint64(0)
        _check(lib().ivfhnsw_gpu_base_value_rows(self._h, lo, hi, C.byref(n)))
        return int(n.value)

    def exact_search_values(self, queries_u8, k, query_ranges):
        """exact_search() with a value interval per query: query_ranges [nq, 2] uint32, (lo, hi) inclusive, (0, VALUE_NONE)
        = no restriction; None is exact_search() itself (ivfhnsw_gpu_exact_search_values)."""
        a, nq, stride = self._exact_queries(queries_u8)
        qr = None if query_ranges is None else _np(query_ranges, np.uint32).reshape(nq, 2)
        dist = np.empty((nq, k), np.float32)
        lab = np.empty((nq, k), np.int64)
        _check(lib().ivfhnsw_gpu_exact_search_values(self._h, nq, C.c_void_p(a.ctypes.data) if nq else None, stride, k,
                                                     _ptr(qr), _ptr(dist), _ptr(lab)))
        return dist, lab

    def exact_search_values_dev(self, nq, d_queries, row_stride, k, d_query_ranges, d_distances, d_labels):
        """The same on device buffers (d_query_ranges: [nq, 2] uint32 in device memory, 8-byte aligned), asynchronous on
        the handle's stream."""
        _check(lib().ivfhnsw_gpu_exact_search_values_dev(self._h, nq, _devptr(d_queries), row_stride, k,
                                                         _devptr(d_query_ranges), _devptr(d_distances), _devptr(d_labels)))

    def exact_range_search_values(self, queries_u8, radius, query_ranges):
        """exact_range_search() with a value interval per query; lims in the caller's query order, results per query in
        ascending label."""
        a, nq, stride = self._exact_queries(queries_u8)
        qr = None if query_ranges is None else _np(query_ranges, np.uint32).reshape(nq, 2)
        lims = np.zeros(nq + 1, np.uint64)
        total = C.c_uint64(0)
        _check(lib().ivfhnsw_gpu_exact_range_search_values(self._h, nq, C.c_void_p(a.ctypes.data) if nq else None, stride,
                                                           _ptr(qr), C.c_float(radius), _ptr(lims), C.byref(total)))
        dist, lab = self.exact_range_results(0, int(total.value))
        return lims, dist, lab

    def exact_range_search_values_dev(self, nq, d_queries, row_stride, d_query_ranges, radius, d_lims):
        """The same on device buffers; returns the number of results, which stay in the handle's memory."""
        total = C.c_uint64(0)
        _check(lib().ivfhnsw_gpu_exact_range_search_values_dev(self._h, nq, _devptr(d_queries), row_stride,
                                                               _devptr(d_query_ranges), C.c_float(radius), _devptr(d_lims),
                                                               C.byref(total)))
        return int(total.value)

    # ---- measurement ---------------------------------------------------------------------------
    def set_profiling(self, on):
        """True / 1: hipEvents around every stage; 2: only around the scan; False / 0: off."""
        _check(lib().ivfhnsw_gpu_set_profiling(self._h, 2 if on == 2 else (1 if on else 0)))

    def reset_stage_ms(self):
        _check(lib().ivfhnsw_gpu_reset_stage_ms(self._h))

    def stage_ms(self):
        out = {}
        for i, name in enumerate(STAGES):
            ms, n = C.c_double(), C.c_uint64()
            _check(lib().ivfhnsw_gpu_get_stage_ms(self._h, i, C.byref(ms), C.byref(n)))
            out[name] = (ms.value, n.value)
        return out

    def last_scan_counts(self):
        a, b = C.c_uint64(), C.c_uint64()
        _check(lib().ivfhnsw_gpu_last_scan_counts(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def last_scan_kernel(self):
        return lib().ivfhnsw_gpu_last_scan_kernel(self._h).decode()

    def memory_bytes(self):
        a = C.c_uint64()
        _check(lib().ivfhnsw_gpu_memory_bytes(self._h, C.byref(a)))
        return a.value


# ---- .bvecs / .fvecs files (utils.h readXvec: records of an int32 dim and dim elements) -------------------------------
def xvecs_shape(path, itemsize):
    """(n, d) of a .bvecs (itemsize 1) / .fvecs (4) file, from its first header and its size."""
    size = os.path.getsize(path)
    with open(path, "rb") as f:
        head = f.read(4)
    d = int(np.frombuffer(head, np.int32)[0]) if len(head) == 4 else 0
    if d <= 0 or size % (4 + d * itemsize):
        raise ValueError("%s: not a %s file of dimension %d" % (path, ".bvecs" if itemsize == 1 else ".fvecs", d))
    return size // (4 + d * itemsize), d


def _check_dims(path, dims, d, first=0, rows=None):
    if (dims != d).any():
        bad = int(np.nonzero(dims != d)[0][0])
        rec = first + bad if rows is None else int(rows[bad])
        raise ValueError("%s: record %d has dimension %d, expected %d" % (path, rec, dims[bad], d))


def open_xvecs(path):
    """Memory-map a .bvecs (uint8) or .fvecs (float32) file: rows [n, d], a read-only view; only the rows a caller
    indexes are read.  read_xvecs checks the dim headers of the rows it returns."""
    itemsize = 1 if path.endswith(".bvecs") else 4
    n, d = xvecs_shape(path, itemsize)
    rec = np.dtype([("dim", "<i4"), ("v", np.uint8 if itemsize == 1 else "<f4", (d,))])
    return np.memmap(path, dtype=rec, mode="r", shape=(n,))


def read_xvecs(path, rows=None):
    """Rows (all, or the sorted index array `rows`) of a .bvecs / .fvecs file, every record's dim header checked."""
    mm = open_xvecs(path)
    d = mm.dtype["v"].shape[0]
    recs = mm if rows is None else mm[np.asarray(rows)]
    _check_dims(path, np.asarray(recs["dim"]), d, rows=rows)
    return np.ascontiguousarray(recs["v"])


def write_fvecs(path, x):
    """x [n, d] as a .fvecs file: what build_quantizer (IndexIVF_HNSW.cpp:34-66) reads as the centroids."""
    x = np.ascontiguousarray(x, np.float32)
    n, d = x.shape
    rec = np.empty(n, np.dtype([("dim", "<i4"), ("v", "<f4", (d,))]))
    rec["dim"] = d
    rec["v"] = x
    rec.tofile(path)


# ---- coarse centroids -------------------------------------------------------------------------------------------------
def learn_centroids(x, nc, niter=10, seed=1234, max_points_per_centroid=256, device=0):
    """nc coarse centroids of x [n, d] (uint8 or float; a memory map is read only where sampled) by exact Lloyd k-means
    on the device (ivfhnsw_gpu_kmeans): at most nc * max_points_per_centroid rows, drawn without replacement (faiss's
    rule), in file order; seeds = nc distinct rows of that sample; both draws from numpy.random.default_rng(seed).
    Returns (centroids f32 [nc, d], obj f64 [niter])."""
    n = len(x)
    if not 1 <= nc <= n:
        raise ValueError("need 1 <= nc <= n (nc %d, n %d)" % (nc, n))
    rng = np.random.default_rng(seed)
    cap = nc * max_points_per_centroid
    if n > cap:
        pick = np.sort(rng.choice(n, size=cap, replace=False))
        xs = np.asarray(x[pick], np.float32)
    else:
        xs = np.asarray(x, np.float32)
    xs = np.ascontiguousarray(xs)
    seeds = xs[rng.choice(len(xs), size=nc, replace=False)]
    g = GpuIndex(device)
    try:
        c, _, obj = g.kmeans(xs, seeds, niter)
    finally:
        g.close()
    return c, obj
