"""fleetrec_amd -- Python host binding of the MI355X-native FleetRec hot path.

A thin ctypes mirror of include/fleetrec.h (the C-ABI in libfleetrec.so).  It exists for the test
harness and bench.py; the production host is the C++ driver (the counterpart of the reference's
GPU/final_network_cublasLt_1_node_no_FIFO_scatter/cuda_server.c).  There is no silent CPU fallback: if the
HIP library is missing, or a context is asked for on a device that is not a visible gfx950, calls raise
FleetRecError; Context(model, device=DEVICE_CPU) asks for the library's own CPU back-end explicitly.

Vocabulary follows the reference: tables, banks, rounds, records (the per-item concatenated
feature vector the FPGA sends), workers (thread_consume), batches.
"""
import contextlib
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("FR_LIB") or os.path.join(_HERE, "libfleetrec.so")   # FR_LIB: A/B experiments load another build of the same ABI

FR_OK, FR_ERR_INVALID, FR_ERR_NO_DEVICE, FR_ERR_OOM, FR_ERR_HIP, FR_ERR_INDEX_RANGE, FR_ERR_STATE, FR_ERR_COMM = 0, -1, -2, -3, -4, -5, -6, -7
MODEL_A, MODEL_B, MODEL_C = 0, 1, 2
FILL_EVEN_ODD, FILL_HASH, FILL_TAGGED = 0, 1, 2
WEIGHTS_ONES, WEIGHTS_UNIFORM = 0, 1
FC_FP32, FC_BF16, FC_FP8 = 0, 1, 2
ACT_NONE, ACT_RELU = 0, 1   # fr_ctx_set_epilogue (fleetrec_serving.h)
_ACTS = {"none": ACT_NONE, "relu": ACT_RELU}
LAYOUT_SEMANTIC, LAYOUT_BLOCKED = 0, 1
INDEX_PER_TABLE, INDEX_PER_ITEM, INDEX_PER_BANK = 0, 1, 2
SEG_TABLE, SEG_COPY, SEG_DENSE = 0, 1, 2
GATHER_WORD_MAJOR, GATHER_ITEM_TILE, GATHER_ITEM_TILE_DEDUP, GATHER_ITEM_TILE_DEDUP_COUNT, GATHER_WORD_MAJOR_ONE_CHUNK = 0, 1, 2, 3, 4
EXCHANGE_ALLGATHER, EXCHANGE_ALLTOALL = 0, 1   # fr_exchange: how a sharded step's slices travel (Comm.set_exchange)
POOL_MAX_HOTS = 64   # FR_POOL_MAX_HOTS (fleetrec_serving.h): slots per bag of a pooled lookup
TOPK_MAX_K = 256   # FR_TOPK_MAX_K (fleetrec_serving.h): the largest k of a top-K ranking
REQ_ONE_HOT, REQ_POOLED, REQ_DENSE = 0, 1, 2   # FR_REQ_* (fleetrec_serving.h): the forms of a request-form expansion
KEYS_ROWS, KEYS_HASHED, KEYS_MAPPED = 0, 1, 2   # FR_KEYS_*: the key space of an index column (Context.set_key_space)
KEY_EMPTY, KEY_NO_ROW = -1, 0x7fffffff   # FR_KEY_EMPTY: the empty slot of a bag; FR_KEY_NO_ROW: the row of a key without one (out of range for every gather)
KEY_ROWS_FULL, KEY_ROWS_REQUEST, KEY_ROWS_CANDIDATE = 0, 1, 2   # FR_KEY_ROWS_*: which rows Worker.resolve_keys_device resolves
POOL_SUM, POOL_MEAN = 0, 1   # FR_POOL_SUM / FR_POOL_MEAN: the pooling mode of an index column (Context.set_pooling(hots, modes))
ABI_VERSION = 6   # include/fleetrec.h FR_ABI_VERSION this binding was written against
MEM_CLASS_NAMES = {0: "HBM", 1: "DDR", 2: "PLRAM"}


class TableDesc(ctypes.Structure):
    _fields_ = [("mem_class", ctypes.c_int32), ("table_id", ctypes.c_int32), ("source", ctypes.c_int32),
                ("dim", ctypes.c_int32), ("rows", ctypes.c_int64), ("bank", ctypes.c_int32),
                ("round", ctypes.c_int32), ("addr_axi", ctypes.c_int64)]


class Segment(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_int32), ("src", ctypes.c_int32), ("src_col", ctypes.c_int32),
                ("rec_offset", ctypes.c_int32), ("len", ctypes.c_int32), ("source", ctypes.c_int32)]


class ModelDesc(ctypes.Structure):
    _fields_ = [("name", ctypes.c_char * 32), ("n_tables", ctypes.c_int32), ("n_segments", ctypes.c_int32),
                ("tables", ctypes.POINTER(TableDesc)), ("segments", ctypes.POINTER(Segment)),
                ("record_len", ctypes.c_int32), ("dense_len", ctypes.c_int32), ("fc", ctypes.c_int32 * 5),
                ("layout", ctypes.c_int32), ("index_mode", ctypes.c_int32)]


class FleetRecError(RuntimeError):
    def __init__(self, status, message):
        super().__init__("fleetrec status %d: %s" % (status, message))
        self.status = status


_lib = None

# every symbol include/fleetrec.h, fleetrec_serving.h and fleetrec_diag.h declare (the not-gpu test checks the .so exports all of them)
ABI_SYMBOLS = [
    "fr_abi_version", "fr_last_error", "fr_device_count", "fr_cpu_set_threads", "fr_ctx_set_chain_width", "fr_ctx_chain_width", "fr_model_builtin", "fr_model_clone_scaled", "fr_model_free",
    "fr_model_table_bytes", "fr_model_index_cols", "fr_model_bank_map", "fr_ctx_set_gather_variant", "fr_ctx_gather_variant",
    "fr_ctx_gather_merged_lookups", "fr_ctx_gather_groups", "fr_comm_unique_id", "fr_comm_init_rank", "fr_comm_init_all", "fr_comm_destroy", "fr_comm_set_wait_ms",
    "fr_worker_submit_sharded", "fr_worker_calibrate_fp8_sharded", "fr_ctx_create", "fr_ctx_create_sharded", "fr_ctx_destroy", "fr_ctx_model",
    "fr_ctx_fill_tables", "fr_ctx_upload_table", "fr_ctx_download_table", "fr_ctx_set_weights", "fr_ctx_fill_weights",
    "fr_ctx_get_weights", "fr_ctx_set_fc_precision", "fr_ctx_get_fp8_exponents", "fr_ctx_set_fp8_act_exponents",
    "fr_worker_calibrate_fp8", "fr_worker_calibrate_fp8_slices", "fr_worker_push_host", "fr_worker_stage_acquire", "fr_worker_push_staged", "fr_worker_flush", "fr_worker_host_poll", "fr_worker_host_pending", "fr_ctx_set_small_block", "fr_worker_stream", "fr_worker_gather_slices", "fr_worker_fc_from_slices_lp", "fr_worker_create", "fr_worker_destroy", "fr_worker_idx_ptr",
    "fr_worker_dense_ptr", "fr_worker_score_ptr", "fr_worker_submit", "fr_worker_submit_device", "fr_worker_push_device", "fr_worker_push_device_list", "fr_worker_sync",
    "fr_worker_gather_only", "fr_worker_fc_only", "fr_worker_fc_layer_only", "fr_worker_fc_layer_repeat", "fr_worker_records_dptr", "fr_worker_features_dptr", "fr_worker_timer_start",
    "fr_worker_timer_stop_ms", "fr_device_malloc", "fr_device_free", "fr_memcpy_h2d", "fr_memcpy_d2h",
    "fr_device_synchronize", "fr_ctx_shard_info", "fr_driver_create", "fr_driver_destroy", "fr_driver_run_resident",
    "fr_driver_worker", "fr_driver_score_ring", "fr_driver_run_host", "fr_driver_run_host_streaming", "fr_driver_host_score_ring", "fr_ctx_stream_group", "fr_ctx_set_stream_group", "fr_model_shard_plan", "fr_worker_fc_from_slices", "fr_worker_last_kernel", "fr_worker_inject_fc_failure", "fr_ctx_set_lp_bank_image", "fr_ctx_lp_bank_image_bytes",
    "fr_comm_set_exchange", "fr_comm_exchange", "fr_comm_exchange_bytes",
    "fr_ctx_set_pooling", "fr_ctx_pooled_index_cols", "fr_worker_gather_pooled", "fr_worker_submit_pooled_device", "fr_worker_submit_pooled",
    "fr_ctx_set_pooling_modes", "fr_ctx_pooling_mode", "fr_worker_gather_pooled_weighted", "fr_worker_submit_pooled_weighted_device", "fr_worker_pool_weights_ptr",
    "fr_worker_submit_pooled_weighted",
    "fr_worker_gather_pooled_csr", "fr_worker_submit_pooled_csr_device", "fr_worker_pool_offsets_ptr", "fr_worker_submit_pooled_csr",
    "fr_worker_update_rows", "fr_ctx_update_rows", "fr_ctx_lp_bank_image_builds",
    "fr_worker_push_pooled_device", "fr_worker_push_pooled_csr_device", "fr_worker_push_pooled_device_list",
    "fr_ctx_create_sharded_pooled", "fr_worker_gather_slices_pooled", "fr_worker_gather_slices_pooled_csr", "fr_worker_submit_sharded_pooled",
    "fr_worker_submit_sharded_pooled_csr", "fr_worker_calibrate_fp8_sharded_pooled",
    "fr_worker_topk_device", "fr_worker_topk",
    "fr_ctx_set_request_columns", "fr_ctx_request_words", "fr_worker_expand_requests_device", "fr_worker_request_idx_ptr",
    "fr_worker_request_weights_ptr", "fr_worker_request_dense_ptr", "fr_worker_request_offsets_ptr", "fr_worker_submit_requests",
    "fr_ctx_set_key_space", "fr_ctx_key_space", "fr_ctx_put_keys", "fr_worker_put_keys", "fr_worker_resolve_keys_device", "fr_worker_key_ptr",
    "fr_worker_submit_keyed", "fr_worker_key_misses",
    "fr_worker_erase_keys", "fr_ctx_erase_keys", "fr_ctx_key_space_stats", "fr_ctx_export_keys", "fr_ctx_rebuild_key_space",
    "fr_ctx_set_row_pool", "fr_ctx_row_pool", "fr_worker_admit_keys", "fr_ctx_admit_keys",
    "fr_ctx_set_epilogue", "fr_ctx_epilogue",
]


# the entry points ABI 6 gained last (pooling modes and per-sample weights, sparse row updates, the offsets form of the pooled lookups, their streaming pushes): the only names an FR_LIB build of the same ABI may lack
_ADDED_IN_ABI_6 = ("fr_worker_update_rows", "fr_ctx_update_rows", "fr_ctx_lp_bank_image_builds",
                   "fr_ctx_set_pooling_modes", "fr_ctx_pooling_mode", "fr_worker_gather_pooled_weighted", "fr_worker_submit_pooled_weighted_device",
                   "fr_worker_pool_weights_ptr", "fr_worker_submit_pooled_weighted",
                   "fr_worker_gather_pooled_csr", "fr_worker_submit_pooled_csr_device", "fr_worker_pool_offsets_ptr", "fr_worker_submit_pooled_csr",
                   "fr_worker_push_pooled_device", "fr_worker_push_pooled_csr_device", "fr_worker_push_pooled_device_list",
                   "fr_ctx_create_sharded_pooled", "fr_worker_gather_slices_pooled", "fr_worker_gather_slices_pooled_csr", "fr_worker_submit_sharded_pooled",
                   "fr_worker_submit_sharded_pooled_csr", "fr_worker_calibrate_fp8_sharded_pooled",
                   "fr_worker_topk_device", "fr_worker_topk",
                   "fr_ctx_set_request_columns", "fr_ctx_request_words", "fr_worker_expand_requests_device", "fr_worker_request_idx_ptr",
                   "fr_worker_request_weights_ptr", "fr_worker_request_dense_ptr", "fr_worker_request_offsets_ptr", "fr_worker_submit_requests",
                   "fr_ctx_set_key_space", "fr_ctx_key_space", "fr_ctx_put_keys", "fr_worker_put_keys", "fr_worker_resolve_keys_device", "fr_worker_key_ptr",
                   "fr_worker_submit_keyed", "fr_worker_key_misses",
                   "fr_worker_erase_keys", "fr_ctx_erase_keys", "fr_ctx_key_space_stats", "fr_ctx_export_keys", "fr_ctx_rebuild_key_space",
                   "fr_ctx_set_row_pool", "fr_ctx_row_pool", "fr_worker_admit_keys", "fr_ctx_admit_keys",
                   "fr_ctx_set_epilogue", "fr_ctx_epilogue")


def lib():
    """Load libfleetrec.so (fails loudly when it has not been built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise FleetRecError(FR_ERR_STATE, "HIP library %s not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                            "or `make -C gpu-fpga-recommendation-system_amd/csrc`" % LIB_PATH)
    L = ctypes.CDLL(LIB_PATH)
    vp, i32, i64, u32, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_uint32, ctypes.c_size_t
    pf, pi = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int32)
    sig = {
        "fr_abi_version": (i32, []), "fr_last_error": (ctypes.c_char_p, []), "fr_device_count": (i32, []), "fr_cpu_set_threads": (i32, [i32]), "fr_ctx_set_chain_width": (i32, [vp, i32]), "fr_ctx_chain_width": (i32, [vp]),
        "fr_model_builtin": (ctypes.POINTER(ModelDesc), [i32]),
        "fr_model_clone_scaled": (i32, [ctypes.POINTER(ModelDesc), ctypes.c_double, i64, i64, ctypes.POINTER(ctypes.POINTER(ModelDesc))]),
        "fr_model_free": (None, [ctypes.POINTER(ModelDesc)]),
        "fr_model_table_bytes": (i64, [ctypes.POINTER(ModelDesc)]),
        "fr_model_index_cols": (i32, [ctypes.POINTER(ModelDesc)]),
        "fr_model_bank_map": (i32, [ctypes.POINTER(ModelDesc), pi, ctypes.POINTER(ctypes.c_int64)]),
        "fr_ctx_create": (i32, [ctypes.POINTER(ModelDesc), i32, ctypes.POINTER(vp)]),
        "fr_ctx_create_sharded": (i32, [ctypes.POINTER(ModelDesc), i32, i32, i32, ctypes.POINTER(vp)]),
        "fr_ctx_destroy": (None, [vp]), "fr_ctx_model": (ctypes.POINTER(ModelDesc), [vp]),
        "fr_ctx_fill_tables": (i32, [vp, i32, u32]),
        "fr_ctx_upload_table": (i32, [vp, i32, i64, i64, vp]), "fr_ctx_download_table": (i32, [vp, i32, i64, i64, vp]),
        "fr_ctx_set_weights": (i32, [vp, i32, vp, sz]), "fr_ctx_fill_weights": (i32, [vp, i32, u32]),
        "fr_ctx_get_weights": (i32, [vp, i32, vp, sz]), "fr_ctx_set_fc_precision": (i32, [vp, i32]),
        "fr_ctx_get_fp8_exponents": (i32, [vp, vp, vp]), "fr_ctx_set_fp8_act_exponents": (i32, [vp, vp]),
        "fr_worker_push_host": (i32, [vp, i32, vp, vp, vp]), "fr_worker_stream": (vp, [vp]),
        "fr_worker_stage_acquire": (i32, [vp, i32, ctypes.POINTER(vp), ctypes.POINTER(vp)]), "fr_worker_push_staged": (i32, [vp, i32, vp]),
        "fr_ctx_set_small_block": (i32, [vp, i32]), "fr_worker_flush": (i32, [vp]), "fr_worker_host_poll": (i32, [vp, ctypes.POINTER(ctypes.c_longlong)]),
        "fr_worker_host_pending": (i32, [vp, ctypes.POINTER(i32), ctypes.POINTER(i32), ctypes.POINTER(i32)]),
        "fr_worker_gather_slices": (i32, [vp, i32, vp, vp, vp, i32]), "fr_worker_fc_from_slices_lp": (i32, [vp, i32, i32, i32, vp, i32, vp]),
        "fr_worker_calibrate_fp8": (i32, [vp, i32]), "fr_worker_calibrate_fp8_slices": (i32, [vp, i32, i32, i32, vp]),
        "fr_worker_create": (i32, [vp, i32, ctypes.POINTER(vp)]), "fr_worker_destroy": (None, [vp]),
        "fr_worker_idx_ptr": (pi, [vp]), "fr_worker_dense_ptr": (pf, [vp]), "fr_worker_score_ptr": (pf, [vp]),
        "fr_worker_submit": (i32, [vp, i32]), "fr_worker_submit_device": (i32, [vp, i32, vp, vp, vp]), "fr_worker_push_device": (i32, [vp, i32, vp, vp, vp]), "fr_worker_push_device_list": (i32, [vp, i32, vp, vp, vp, vp]),
        "fr_worker_sync": (i32, [vp]), "fr_worker_gather_only": (i32, [vp, i32, vp, vp, vp]),
        "fr_worker_fc_only": (i32, [vp, i32, vp, vp]), "fr_worker_fc_layer_only": (i32, [vp, i32, i32]), "fr_worker_fc_layer_repeat": (i32, [vp, i32, i32, i32]), "fr_worker_records_dptr": (vp, [vp]),
        "fr_worker_features_dptr": (vp, [vp, ctypes.POINTER(ctypes.c_int)]),
        "fr_worker_timer_start": (i32, [vp]), "fr_worker_timer_stop_ms": (i32, [vp, pf]),
        "fr_device_malloc": (i32, [vp, sz, ctypes.POINTER(vp)]), "fr_device_free": (i32, [vp, vp]),
        "fr_memcpy_h2d": (i32, [vp, vp, vp, sz]), "fr_memcpy_d2h": (i32, [vp, vp, vp, sz]),
        "fr_device_synchronize": (i32, [vp]),
        "fr_ctx_shard_info": (i32, [vp] + [ctypes.POINTER(ctypes.c_int)] * 5),
        "fr_driver_create": (i32, [vp, i32, i32, i32, ctypes.POINTER(vp)]), "fr_driver_destroy": (None, [vp]),
        "fr_driver_run_resident": (i32, [vp, i32, i64, ctypes.POINTER(vp), ctypes.POINTER(vp), i32, ctypes.POINTER(ctypes.c_double)]),
        "fr_driver_worker": (vp, [vp, i32, i32]), "fr_driver_score_ring": (vp, [vp, i32, i32, ctypes.POINTER(ctypes.c_int)]),
        "fr_ctx_stream_group": (i32, [vp]), "fr_ctx_set_stream_group": (i32, [vp, i32]),
        "fr_ctx_set_gather_variant": (i32, [vp, i32]), "fr_ctx_gather_variant": (i32, [vp]),
        "fr_comm_unique_id": (i32, [vp]), "fr_comm_init_rank": (i32, [vp, vp, ctypes.POINTER(vp)]),
        "fr_comm_init_all": (i32, [ctypes.POINTER(vp), i32, ctypes.POINTER(vp)]), "fr_comm_destroy": (None, [vp]), "fr_comm_set_wait_ms": (i32, [vp, i32]),
        "fr_worker_submit_sharded": (i32, [vp, vp, i32]), "fr_worker_calibrate_fp8_sharded": (i32, [vp, vp, i32]),
        "fr_ctx_gather_merged_lookups": (i32, [vp, ctypes.POINTER(ctypes.c_uint64), i32]),
        "fr_ctx_gather_groups": (i32, [vp, ctypes.POINTER(ctypes.c_int)]),
        "fr_driver_run_host": (i32, [vp, i32, i64, ctypes.POINTER(vp), ctypes.POINTER(vp), i32, ctypes.POINTER(ctypes.c_double)]),
        "fr_driver_run_host_streaming": (i32, [vp, i32, i64, ctypes.POINTER(vp), ctypes.POINTER(vp), i32, ctypes.POINTER(ctypes.c_double)]),
        "fr_driver_host_score_ring": (vp, [vp, i32, i32, ctypes.POINTER(ctypes.c_int)]),
        "fr_model_shard_plan": (i32, [ctypes.POINTER(ModelDesc), i32, pi, pi, ctypes.POINTER(ctypes.c_int)]),
        "fr_worker_fc_from_slices": (i32, [vp, i32, i32, i32, vp, vp]),
        "fr_worker_last_kernel": (ctypes.c_char_p, [vp]), "fr_worker_inject_fc_failure": (i32, [vp, i32]),
        "fr_ctx_set_lp_bank_image": (i32, [vp, i32]), "fr_ctx_lp_bank_image_bytes": (ctypes.c_size_t, [vp]),
        "fr_comm_set_exchange": (i32, [vp, i32]), "fr_comm_exchange": (i32, [vp]),
        "fr_comm_exchange_bytes": (i32, [vp, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]),
        "fr_ctx_set_pooling": (i32, [vp, pi, i32]), "fr_ctx_pooled_index_cols": (i32, [vp]),
        "fr_worker_gather_pooled": (i32, [vp, i32, vp, vp, vp]), "fr_worker_submit_pooled_device": (i32, [vp, i32, vp, vp, vp]),
        "fr_worker_submit_pooled": (i32, [vp, i32]),
        "fr_ctx_set_pooling_modes": (i32, [vp, pi, i32]), "fr_ctx_pooling_mode": (i32, [vp, i32]),
        "fr_worker_gather_pooled_weighted": (i32, [vp, i32, vp, vp, vp, vp]), "fr_worker_submit_pooled_weighted_device": (i32, [vp, i32, vp, vp, vp, vp]),
        "fr_worker_pool_weights_ptr": (pf, [vp]), "fr_worker_submit_pooled_weighted": (i32, [vp, i32]),
        "fr_worker_gather_pooled_csr": (i32, [vp, i32, vp, vp, i64, vp, vp, vp]), "fr_worker_submit_pooled_csr_device": (i32, [vp, i32, vp, vp, i64, vp, vp, vp]),
        "fr_worker_push_pooled_device": (i32, [vp, i32, vp, vp, vp, vp]), "fr_worker_push_pooled_csr_device": (i32, [vp, i32, vp, vp, i64, vp, vp, vp]),
        "fr_worker_push_pooled_device_list": (i32, [vp, i32, vp, vp, vp, vp, vp]),
        "fr_worker_pool_offsets_ptr": (pi, [vp]), "fr_worker_submit_pooled_csr": (i32, [vp, i32, i32]),
        "fr_worker_update_rows": (i32, [vp, i32, i32, vp, vp]), "fr_ctx_update_rows": (i32, [vp, i32, i32, vp, vp]),
        "fr_ctx_lp_bank_image_builds": (ctypes.c_longlong, [vp]),
        "fr_ctx_create_sharded_pooled": (i32, [ctypes.POINTER(ModelDesc), i32, i32, i32, pi, pi, i32, ctypes.POINTER(vp)]),
        "fr_worker_gather_slices_pooled": (i32, [vp, i32, vp, vp, vp, vp, i32]),
        "fr_worker_gather_slices_pooled_csr": (i32, [vp, i32, vp, vp, i64, vp, vp, vp, i32]),
        "fr_worker_submit_sharded_pooled": (i32, [vp, vp, i32, i32]), "fr_worker_submit_sharded_pooled_csr": (i32, [vp, vp, i32, i32]),
        "fr_worker_calibrate_fp8_sharded_pooled": (i32, [vp, vp, i32, i32]),
        "fr_worker_topk_device": (i32, [vp, i32, vp, i32, vp, i32, vp, vp]), "fr_worker_topk": (i32, [vp, i32, i32, vp, i32, vp, vp]),
        "fr_ctx_set_request_columns": (i32, [vp, pi, i32, i32]), "fr_ctx_request_words": (i32, [vp, i32, ctypes.POINTER(i32), ctypes.POINTER(i32), ctypes.POINTER(i32)]),
        "fr_worker_expand_requests_device": (i32, [vp, i32, i32, vp, vp, vp, i32, vp]),
        "fr_worker_request_idx_ptr": (pi, [vp]), "fr_worker_request_weights_ptr": (pf, [vp]), "fr_worker_request_dense_ptr": (pf, [vp]),
        "fr_worker_request_offsets_ptr": (pi, [vp]), "fr_worker_submit_requests": (i32, [vp, i32, i32, i32]),
        "fr_ctx_set_key_space": (i32, [vp, i32, i32, ctypes.c_uint64, i64, ctypes.c_int32]),
        "fr_ctx_key_space": (i32, [vp, i32, ctypes.POINTER(i32), ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(i64), ctypes.POINTER(i64), ctypes.POINTER(ctypes.c_int32)]),
        "fr_ctx_put_keys": (i32, [vp, i32, i32, vp, vp]), "fr_worker_put_keys": (i32, [vp, i32, i32, vp, vp]),
        "fr_worker_resolve_keys_device": (i32, [vp, i32, i32, i32, vp, vp]), "fr_worker_key_ptr": (ctypes.POINTER(ctypes.c_int64), [vp]),
        "fr_worker_submit_keyed": (i32, [vp, i32, i32]), "fr_worker_key_misses": (i32, [vp, ctypes.POINTER(ctypes.c_uint64), i32]),
        "fr_worker_erase_keys": (i32, [vp, i32, i32, vp]), "fr_ctx_erase_keys": (i32, [vp, i32, i32, vp]),
        "fr_ctx_key_space_stats": (i32, [vp, i32, ctypes.POINTER(i64), ctypes.POINTER(i64), ctypes.POINTER(i64), ctypes.POINTER(i64)]),
        "fr_ctx_export_keys": (i32, [vp, i32, i64, vp, vp, ctypes.POINTER(i64)]),
        "fr_ctx_rebuild_key_space": (i32, [vp, i32, ctypes.c_uint64, i64]),
        "fr_ctx_set_row_pool": (i32, [vp, i32, ctypes.c_int32, ctypes.c_int32]),
        "fr_ctx_row_pool": (i32, [vp, i32, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(i64)]),
        "fr_worker_admit_keys": (i32, [vp, i32, i32, vp, vp]), "fr_ctx_admit_keys": (i32, [vp, i32, i32, vp, vp]),
        "fr_ctx_set_epilogue": (i32, [vp, i32, vp, sz, i32]), "fr_ctx_epilogue": (i32, [vp, i32, vp, sz, ctypes.POINTER(i32), ctypes.POINTER(i32)]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(L, name, None)
        if fn is None and name in _ADDED_IN_ABI_6 and os.environ.get("FR_LIB"):
            continue   # an FR_LIB build of ABI 6 from before these additive entry points (an A/B run against an older commit): calling one fails
        if fn is None:
            raise FleetRecError(FR_ERR_STATE, "%s does not export %s: rebuild it (make -C gpu-fpga-recommendation-system_amd/csrc)" % (LIB_PATH, name))
        fn.restype, fn.argtypes = res, args
    got = L.fr_abi_version()
    if got != ABI_VERSION:   # an FR_LIB build of another ABI would be called with the wrong contract
        raise FleetRecError(FR_ERR_STATE, "%s reports ABI version %d, this binding needs %d" % (LIB_PATH, got, ABI_VERSION))
    _lib = L
    return L


def bags_to_csr(padded_idx, hots, weights=None, keep_empty=False):
    """The padded rectangle of the pooled lookups (int32 [B][sum(hots)], -1 = empty slot; weights float32 of the same shape or None) ->
    (offsets int32 [B * C + 1], indices int32 [nnz], weights float32 [nnz] or None): the same bags in the offsets form, item-major and
    column-minor, every bag's entries in slot order.  The -1 slots are dropped unless keep_empty (then every bag keeps its hots[c] slots)."""
    idx = np.ascontiguousarray(np.asarray(padded_idx, dtype=np.int32).reshape(len(padded_idx), -1))
    hots = np.asarray(hots, dtype=np.int64).reshape(-1)
    if idx.shape[1] != int(hots.sum()):
        raise FleetRecError(FR_ERR_INVALID, "padded index rows have %d columns, hots sum to %d" % (idx.shape[1], int(hots.sum())))
    keep = np.ones(idx.shape, bool) if keep_empty else idx != -1
    if len(hots) == 0 or int(hots.min()) < 1:
        raise FleetRecError(FR_ERR_INVALID, "hots must be at least 1 for every index column")
    pre = np.concatenate([[0], np.cumsum(hots)[:-1]])                 # every column's first padded slot: its slots are contiguous
    lens = np.add.reduceat(keep, pre, axis=1, dtype=np.int64)       # [B][C]: the kept slots of every bag
    offsets = np.zeros(lens.size + 1, np.int64)
    np.cumsum(lens.reshape(-1), out=offsets[1:])
    if int(offsets[-1]) > np.iinfo(np.int32).max:
        raise FleetRecError(FR_ERR_INVALID, "%d entries do not fit int32 offsets" % int(offsets[-1]))
    w = None
    if weights is not None:
        w = np.ascontiguousarray(np.asarray(weights, dtype=np.float32).reshape(idx.shape))[keep]
    return offsets.astype(np.int32), idx[keep], w


def _check(status):
    if status != FR_OK:
        raise FleetRecError(status, lib().fr_last_error().decode("utf-8", "replace"))


def device_count():
    return lib().fr_device_count()


DEVICE_CPU = -1   # Context(model, device=DEVICE_CPU): the library's CPU back-end (fp32 only; include/fleetrec.h fr_ctx_create)


def cpu_set_threads(n=0):
    """Host threads of the CPU back-end (0 = every usable core) -> the number in use."""
    r = lib().fr_cpu_set_threads(n)
    if r < 0:
        _check(r)
    return r


class Model:
    """A model description (built-in A/B/C, or a row-scaled clone)."""

    def __init__(self, ptr, owned=False, keepalive=None):
        self._ptr, self._owned, self._keep = ptr, owned, keepalive

    @classmethod
    def builtin(cls, which):
        p = lib().fr_model_builtin(which)
        if not p:
            _check(FR_ERR_INVALID)
        return cls(p)

    @classmethod
    def from_spec(cls, spec):
        """Build a user-defined model from a plain dict (the run-time counterpart of the reference's generated
        constants.hpp, FPGA/kernel/user_krnl/embedding_47_krnl/src/hls/constants.hpp:28,505):

            {"name": "my_model",
             "tables": [{"dim": 8, "rows": 100000, "class": "HBM", "bank": 0}, ...],   # listed in record (wire) order; tables with
                                                                                # equal (class, bank) share a memory bank (default: own bank)
             "dense_len": 0,                                                    # floats per item supplied by the request
             "dense_at": 0,                                                     # table position the dense block precedes
             "pad": [{"after_table": 3, "copy_of": 1, "col": 0}],               # optional 4-float COPY pads
             "fc": [1024, 512, 256]}                                            # hidden widths; K = record length, OUT = 1

        The description is validated by the library (fr_model_clone_scaled -> fr_model_validate)."""
        tabs_in = spec["tables"]
        n = len(tabs_in)
        tabs = (TableDesc * n)()
        cls_id = {"HBM": 0, "DDR": 1, "PLRAM": 2}
        for t, d in enumerate(tabs_in):
            tabs[t] = TableDesc(mem_class=cls_id.get(d.get("class", "HBM"), 0), table_id=t % 256, source=0, dim=int(d["dim"]),
                                rows=int(d["rows"]), bank=int(d.get("bank", t)), round=0, addr_axi=0)
        dense_len, dense_at = int(spec.get("dense_len", 0)), int(spec.get("dense_at", 0))
        pads = {int(p_["after_table"]): p_ for p_ in spec.get("pad", [])}
        segs, pos, seen_dense = [], 0, False
        for t in range(n + 1):
            if dense_len and t == dense_at:
                segs.append((SEG_DENSE, -1, 0, pos, dense_len, 2))
                pos += dense_len
                seen_dense = True
            if t == n:
                break
            src_id = 1 if seen_dense else 0
            segs.append((SEG_TABLE, t, 0, pos, int(tabs_in[t]["dim"]), src_id))
            pos += int(tabs_in[t]["dim"])
            if t in pads:
                segs.append((SEG_COPY, int(pads[t]["copy_of"]), int(pads[t].get("col", 0)), pos, 4, src_id))
                pos += 4
        S = (Segment * len(segs))(*[Segment(kind=k, src=s_, src_col=c, rec_offset=o, len=l, source=sr) for k, s_, c, o, l, sr in segs])
        d = ModelDesc()
        d.name = spec.get("name", "custom").encode()[:31]
        d.n_tables, d.n_segments = n, len(segs)
        d.tables = ctypes.cast(tabs, ctypes.POINTER(TableDesc))
        d.segments = ctypes.cast(S, ctypes.POINTER(Segment))
        d.record_len, d.dense_len = pos, dense_len
        fcw = [pos] + [int(v) for v in spec["fc"]] + [1]
        if len(fcw) != 5:
            raise FleetRecError(FR_ERR_INVALID, "spec['fc'] must list exactly three hidden widths")
        for i, v in enumerate(fcw):
            d.fc[i] = v
        tmp = cls(ctypes.pointer(d), keepalive=(tabs, S, d))
        return tmp.clone()  # validated deep copy owned by the library

    def placement_report(self, l2_bytes=4 << 20, mall_bytes=256 << 20):
        """Where each table will live on MI355X when accessed uniformly, and what the gather costs per item: the
        MicroRec/FleetRec placement question (on-chip PLRAM vs HBM vs DDR banks) mapped onto L2 / Infinity Cache / HBM.
        A row costs one 128-byte line beyond L2 whatever its size (profiles/archive/r01_experiments.md)."""
        tabs = self.tables()
        order = sorted(range(len(tabs)), key=lambda t: tabs[t].rows * tabs[t].dim * 4)
        cum, out = 0, []
        for t in order:
            b = tabs[t].rows * tabs[t].dim * 4
            cum += b
            level = "L2" if cum <= 8 * l2_bytes else ("InfinityCache" if cum <= mall_bytes else "HBM")
            out.append({"table": t, "class": MEM_CLASS_NAMES[tabs[t].mem_class], "id": tabs[t].table_id, "dim": tabs[t].dim,
                        "rows": tabs[t].rows, "bytes": b, "level": level})
        rows_per_item = len(tabs)
        useful = sum(t.dim * 4 for t in tabs)
        return {"tables": sorted(out, key=lambda e: e["table"]), "table_bytes": cum, "rows_per_item": rows_per_item,
                "useful_row_bytes_per_item": useful, "line_bytes_per_item_beyond_l2": 128 * sum(1 for e in out if e["level"] != "L2"),
                "levels": {lv: sum(1 for e in out if e["level"] == lv) for lv in ("L2", "InfinityCache", "HBM")}}

    def clone(self, row_scale=1.0, min_rows=1, max_rows=0, layout=None, index_mode=None):
        out = ctypes.POINTER(ModelDesc)()
        _check(lib().fr_model_clone_scaled(self._ptr, row_scale, min_rows, max_rows, ctypes.byref(out)))
        m = Model(out, owned=True)
        if layout is not None:
            out.contents.layout = layout
        if index_mode is not None:
            out.contents.index_mode = index_mode
        return m

    def __del__(self):
        if getattr(self, "_owned", False) and self._ptr:
            lib().fr_model_free(self._ptr)
            self._ptr = None

    @property
    def desc(self):
        return self._ptr.contents

    @property
    def name(self):
        return self.desc.name.decode()

    @property
    def n_tables(self):
        return self.desc.n_tables

    @property
    def record_len(self):
        return self.desc.record_len

    @property
    def dense_len(self):
        return self.desc.dense_len

    @property
    def fc(self):
        return list(self.desc.fc)

    @property
    def idx_cols(self):
        """int32 columns of one item's index row: n_tables (PER_TABLE), 1 (PER_ITEM) or the number of banks (PER_BANK)."""
        n = lib().fr_model_index_cols(self._ptr)
        if n <= 0:
            _check(n if n < 0 else FR_ERR_INVALID)
        return n

    def bank_map(self):
        """-> (bank_of_table int32 [n_tables], bank_rows int64 [n_banks]): the memory bank (= index column in PER_BANK mode) of
        every table, banks numbered by first appearance in the table list, and the valid index range of each bank (the smallest
        row count among its tables)."""
        bot = np.empty(self.n_tables, dtype=np.int32)
        rows = np.empty(self.n_tables, dtype=np.int64)
        nb = lib().fr_model_bank_map(self._ptr, bot.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), rows.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)))
        if nb < 0:
            _check(nb)
        return bot, rows[:nb].copy()

    def index_ranges(self):
        """Exclusive upper bound of every index column in the model's index mode (uniform-index generators use this)."""
        mode = self.desc.index_mode
        if mode == INDEX_PER_TABLE:
            return self.rows()
        if mode == INDEX_PER_BANK:
            return self.bank_map()[1]
        return np.array([self.rows().min()], dtype=np.int64)

    def tables(self):
        d = self.desc
        return [d.tables[i] for i in range(d.n_tables)]

    def segments(self):
        d = self.desc
        return [d.segments[i] for i in range(d.n_segments)]

    def rows(self):
        return np.array([t.rows for t in self.tables()], dtype=np.int64)

    def table_bytes(self):
        return lib().fr_model_table_bytes(self._ptr)

    def shard_plan(self, n_shards):
        """-> (slice_offsets, slice_lens, padded_len): the table-ID sharding of the record over n_shards GPUs (host only)."""
        off = (ctypes.c_int32 * n_shards)()
        ln = (ctypes.c_int32 * n_shards)()
        pad = ctypes.c_int()
        _check(lib().fr_model_shard_plan(self._ptr, n_shards, off, ln, ctypes.byref(pad)))
        return list(off), list(ln), pad.value


    def shard_table_bytes(self, n_shards):
        """Table bytes every shard of the n_shards-way plan would hold (host only): a table belongs to the shard whose record slice its
        segments fall in."""
        offs, lens, _ = self.shard_plan(n_shards)
        tabs = self.tables()
        out = [0] * n_shards
        seen = set()
        for sg in self.segments():
            if sg.kind == SEG_DENSE:
                continue
            g = max(i for i in range(n_shards) if offs[i] <= sg.rec_offset)
            if (g, sg.src) not in seen:
                seen.add((g, sg.src))
                out[g] += int(tabs[sg.src].rows) * int(tabs[sg.src].dim) * 4
        return out

    def min_shards(self, hbm_bytes=288e9, reserve=0.10, candidates=(1, 2, 4, 8)):
        """BASELINE.json north_star's rule: tables shard by table-ID over the GPUs of a node ONLY when they do not fit one GPU's HBM.
        -> the smallest G of `candidates` whose largest shard fits (1 - reserve) * hbm_bytes, or None when even the last one does not
        (table-ID sharding cannot split a table)."""
        budget = (1.0 - reserve) * hbm_bytes
        for G in candidates:
            if G <= self.desc.n_segments and max(self.shard_table_bytes(G)) <= budget:
                return G
        return None


_ptr_generation = 0   # bumped whenever any DeviceBuffer's `ptr` changes (free() included): pointer arrays marshalled earlier are stale (Driver._pool_array)


class DeviceBuffer:
    """Raw HBM allocation made through the C-ABI (no torch involved)."""

    @property
    def ptr(self):
        return self._ptr

    @ptr.setter
    def ptr(self, p):
        global _ptr_generation
        _ptr_generation += 1
        self._ptr = p

    def __init__(self, ctx, nbytes):
        self.ctx, self.nbytes = ctx, int(nbytes)
        p = ctypes.c_void_p()
        _check(lib().fr_device_malloc(ctx._h, self.nbytes, ctypes.byref(p)))
        self.ptr = p

    @classmethod
    def from_numpy(cls, ctx, arr):
        arr = np.ascontiguousarray(arr)
        b = cls(ctx, arr.nbytes)
        b.upload(arr)
        return b

    def upload(self, arr):
        arr = np.ascontiguousarray(arr)
        assert arr.nbytes <= self.nbytes
        _check(lib().fr_memcpy_h2d(self.ctx._h, self.ptr, arr.ctypes.data_as(ctypes.c_void_p), arr.nbytes))

    def download(self, dtype, count):
        out = np.empty(count, dtype=dtype)
        assert out.nbytes <= self.nbytes
        _check(lib().fr_memcpy_d2h(self.ctx._h, out.ctypes.data_as(ctypes.c_void_p), self.ptr, out.nbytes))
        return out

    def free(self):
        if self.ptr:
            lib().fr_device_free(self.ctx._h, self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Context:
    """Device + model + tables + weights; shared by all workers (one per GPU)."""

    def __init__(self, model, device=0, shard_rank=0, n_shards=1, hots=None, modes=None):
        """hots (/ modes): pooling stated at creation (fr_ctx_create_sharded_pooled) -- the only way to pool on a sharded context, whose pooling
        never changes afterwards; the arrays of set_pooling, the same on every rank."""
        self.model = model
        h = ctypes.c_void_p()
        if hots is None:
            if modes is not None:
                raise FleetRecError(FR_ERR_INVALID, "pooling modes without hots")
            _check(lib().fr_ctx_create_sharded(model._ptr, device, shard_rank, n_shards, ctypes.byref(h)))
        else:
            hh = np.ascontiguousarray(np.asarray(hots, dtype=np.int32).ravel())
            md = None if modes is None else np.ascontiguousarray(np.asarray(modes, dtype=np.int32).ravel())
            if md is not None and md.size != hh.size:
                raise FleetRecError(FR_ERR_INVALID, "%d pooling modes for %d hots" % (md.size, hh.size))
            pi = ctypes.POINTER(ctypes.c_int32)
            _check(lib().fr_ctx_create_sharded_pooled(model._ptr, device, shard_rank, n_shards, hh.ctypes.data_as(pi),
                                                      md.ctypes.data_as(pi) if md is not None else None, int(hh.size), ctypes.byref(h)))
        self._h = h

    def close(self):
        if self._h:
            lib().fr_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def fill_tables(self, mode, seed=0):
        _check(lib().fr_ctx_fill_tables(self._h, mode, seed))

    def upload_table(self, table, rows_f32, row0=0):
        a = np.ascontiguousarray(rows_f32)
        assert a.dtype in (np.float32, np.uint32)
        nrows = a.shape[0]
        _check(lib().fr_ctx_upload_table(self._h, table, row0, nrows, a.ctypes.data_as(ctypes.c_void_p)))

    def download_table(self, table, row0, nrows, dtype=np.uint32):
        dim = self.model.desc.tables[table].dim
        out = np.empty((nrows, dim), dtype=dtype)
        _check(lib().fr_ctx_download_table(self._h, table, row0, nrows, out.ctypes.data_as(ctypes.c_void_p)))
        return out

    def update_rows(self, table, row_ids, rows_f32):
        """fr_ctx_update_rows, the host form of the sparse row update: row i of rows_f32 (float32 or uint32 bit patterns, [len(row_ids)][dim])
        becomes table row row_ids[i].  Synchronous; legal beside workers in flight; an id outside the table raises FR_ERR_INDEX_RANGE after
        every in-range row was written."""
        ids = np.ascontiguousarray(np.asarray(row_ids, dtype=np.int32).ravel())
        a = np.ascontiguousarray(rows_f32)
        assert a.dtype in (np.float32, np.uint32)
        dim = self.model.desc.tables[table].dim if 0 <= table < self.model.n_tables else -1
        if dim >= 0 and a.shape != (ids.size, dim):
            raise FleetRecError(FR_ERR_INVALID, "rows are %s, %d listed ids of table %d need (%d, %d)" % (a.shape, ids.size, table, ids.size, dim))
        _check(lib().fr_ctx_update_rows(self._h, table, int(ids.size), ids.ctypes.data_as(ctypes.c_void_p), a.ctypes.data_as(ctypes.c_void_p)))

    def lp_bank_image_builds(self):
        """fleetrec_diag.h: full builds of the operand-type bank image so far (an update_rows patch never counts)."""
        return int(lib().fr_ctx_lp_bank_image_builds(self._h))

    def set_weights(self, layer, w_colmajor):
        w = np.ascontiguousarray(w_colmajor, dtype=np.float32).ravel()
        _check(lib().fr_ctx_set_weights(self._h, layer, w.ctypes.data_as(ctypes.c_void_p), w.size))

    def fill_weights(self, mode, seed=0):
        _check(lib().fr_ctx_fill_weights(self._h, mode, seed))

    def get_weights(self, layer):
        fc = self.model.fc
        w = np.empty(fc[layer] * fc[layer + 1], dtype=np.float32)
        _check(lib().fr_ctx_get_weights(self._h, layer, w.ctypes.data_as(ctypes.c_void_p), w.size))
        return w

    def set_epilogue(self, layer, bias=None, act="none"):
        """fleetrec_serving.h fr_ctx_set_epilogue: layer 0..3 computes act(W x + bias).  bias: fc[layer + 1] float32 values or None; act: "none" / "relu"
        (or ACT_NONE / ACT_RELU); the output layer (3) takes "none" only.  (None, "none") restores the layer as it was."""
        a = _ACTS.get(act, act) if isinstance(act, str) else act
        if isinstance(a, str):
            raise FleetRecError(FR_ERR_INVALID, "unknown activation %r (\"none\", \"relu\")" % (act,))
        if bias is None:
            _check(lib().fr_ctx_set_epilogue(self._h, layer, None, 0, int(a)))
            return
        b = np.ascontiguousarray(bias, dtype=np.float32).ravel()
        _check(lib().fr_ctx_set_epilogue(self._h, layer, b.ctypes.data_as(ctypes.c_void_p), b.size, int(a)))

    def epilogue(self, layer):
        """-> (bias float32 [fc[layer + 1]] or None, "none" / "relu") as set by set_epilogue."""
        hb, act = ctypes.c_int(0), ctypes.c_int(0)
        _check(lib().fr_ctx_epilogue(self._h, layer, None, 0, ctypes.byref(hb), ctypes.byref(act)))
        b = None
        if hb.value:
            b = np.empty(self.model.fc[layer + 1], dtype=np.float32)
            _check(lib().fr_ctx_epilogue(self._h, layer, b.ctypes.data_as(ctypes.c_void_p), b.size, None, None))
        return b, {v: k for k, v in _ACTS.items()}[act.value]

    def set_fc_precision(self, precision):
        _check(lib().fr_ctx_set_fc_precision(self._h, precision))

    def fp8_exponents(self):
        """-> (act_exp[4] for X, R1, R2, R3; w_exp[3] for W1..W3): tensor T is stored as e4m3(saturate(T * 2**e))."""
        a, w = (ctypes.c_int * 4)(), (ctypes.c_int * 3)()
        _check(lib().fr_ctx_get_fp8_exponents(self._h, a, w))
        return list(a), list(w)

    def set_fp8_act_exponents(self, act_exp):
        _check(lib().fr_ctx_set_fp8_act_exponents(self._h, (ctypes.c_int * 4)(*[int(v) for v in act_exp])))

    def shard_info(self):
        v = [ctypes.c_int() for _ in range(5)]
        _check(lib().fr_ctx_shard_info(self._h, *[ctypes.byref(x) for x in v]))
        return dict(zip(["shard_rank", "n_shards", "slice_offset", "slice_len", "slice_padded"], [x.value for x in v]))

    def stream_group(self):
        return lib().fr_ctx_stream_group(self._h)

    def set_stream_group(self, batches_per_launch):
        _check(lib().fr_ctx_set_stream_group(self._h, batches_per_launch))

    def set_lp_bank_image(self, on):
        """fleetrec_diag.h: 0 = the in-chain gather of a per-bank bf16 / fp8 context reads the fp32 rows (A/B and parity hook)."""
        _check(lib().fr_ctx_set_lp_bank_image(self._h, int(bool(on))))

    def lp_bank_image_bytes(self):
        return int(lib().fr_ctx_lp_bank_image_bytes(self._h))

    def set_chain_width(self, width):
        """Chain width W (1..4): a chain model's bf16 / fp8 GEMM layers take tiles covering 1 / W of the chip (fr_ctx_set_chain_width)."""
        _check(lib().fr_ctx_set_chain_width(self._h, width))

    def chain_width(self):
        """The context's chain width; 0 while undecided (the first low-precision GEMM-layer launch freezes it)."""
        return lib().fr_ctx_chain_width(self._h)

    def set_small_block(self, max_batches):
        """Host-fed blocks of at most max_batches batches take fr_worker_submit's stage launches instead of the fused kernel (latency)."""
        _check(lib().fr_ctx_set_small_block(self._h, max_batches))

    def set_gather_variant(self, variant):
        """GATHER_WORD_MAJOR (default) / GATHER_ITEM_TILE / GATHER_ITEM_TILE_DEDUP(_COUNT): which kernel fr_worker_gather_only runs."""
        _check(lib().fr_ctx_set_gather_variant(self._h, variant))

    def gather_groups(self):
        """Word ranges [starts[g], starts[g + 1]) the word-major gather deals to the 8 XCD groups (fr_ctx_gather_groups)."""
        st = (ctypes.c_int * 9)()
        _check(lib().fr_ctx_gather_groups(self._h, st))
        return [int(x) for x in st]

    def gather_merged_lookups(self, reset=True):
        v = ctypes.c_uint64()
        _check(lib().fr_ctx_gather_merged_lookups(self._h, ctypes.byref(v), 1 if reset else 0))
        return v.value

    def set_pooling(self, hots, modes=None):
        """Multi-hot pooled lookups (fr_ctx_set_pooling): hots[c] = slots (1..POOL_MAX_HOTS) of index column c, for every index column
        of the model's index mode; None clears.  The pooled index row of an item is int32 [sum(hots)], column by column, slot-minor;
        a slot of -1 is empty; a bag is summed in fp32 in slot order.  modes[c] = POOL_SUM / POOL_MEAN per index column
        (fr_ctx_set_pooling_modes: a MEAN bag is its sum divided by its count of non-empty slots); None = every column SUM."""
        if hots is None:
            _check(lib().fr_ctx_set_pooling(self._h, None, 0))
            return
        h = np.ascontiguousarray(np.asarray(hots, dtype=np.int32).ravel())
        _check(lib().fr_ctx_set_pooling(self._h, h.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), int(h.size)))
        if modes is not None:
            self.set_pooling_modes(modes)

    def set_pooling_modes(self, modes):
        """fr_ctx_set_pooling_modes on a context whose pooling is set: POOL_SUM / POOL_MEAN per index column; None = every column SUM."""
        if modes is None:
            _check(lib().fr_ctx_set_pooling_modes(self._h, None, 0))
            return
        md = np.ascontiguousarray(np.asarray(modes, dtype=np.int32).ravel())
        _check(lib().fr_ctx_set_pooling_modes(self._h, md.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), int(md.size)))

    @property
    def pooling_modes(self):
        """int32 [index columns]: the pooling mode of every index column (all POOL_SUM when no pooling is set)."""
        return np.array([lib().fr_ctx_pooling_mode(self._h, c) for c in range(self.model.idx_cols)], dtype=np.int32)

    @property
    def pooled_index_cols(self):
        """P = sum of hots: int32 columns of one item's pooled index row; 0 when no pooling is set."""
        return int(lib().fr_ctx_pooled_index_cols(self._h))

    def set_request_columns(self, shared, dense_shared=False):
        """Request-form batches (fr_ctx_set_request_columns): shared[c] = 1 when index column c belongs to the request (one row per request), 0 when
        it stays per item, for every index column of the model's index mode; dense_shared: the dense features are the request's too.  None clears."""
        if shared is None:
            _check(lib().fr_ctx_set_request_columns(self._h, None, 0, 0))
            return
        sh = np.ascontiguousarray(np.asarray(shared, dtype=np.int32).ravel())
        _check(lib().fr_ctx_set_request_columns(self._h, sh.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), int(sh.size), int(dense_shared)))

    def request_words(self, form):
        """-> (request words, candidate words, row words) of a form (REQ_ONE_HOT, REQ_POOLED, REQ_DENSE): fr_ctx_request_words."""
        r, c, w = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        _check(lib().fr_ctx_request_words(self._h, int(form), ctypes.byref(r), ctypes.byref(c), ctypes.byref(w)))
        return r.value, c.value, w.value

    def set_key_space(self, col, mode, seed=0, max_keys=0, miss_row=KEY_NO_ROW):
        """fr_ctx_set_key_space: what a key of index column `col` means -- KEYS_ROWS (a key is a row), KEYS_HASHED (the hashing trick under `seed`) or
        KEYS_MAPPED (an exact map in device memory, created EMPTY for up to max_keys keys; an absent key resolves to miss_row: a row of the column,
        -1 = an empty bag slot, or KEY_NO_ROW = an index-range error at sync)."""
        _check(lib().fr_ctx_set_key_space(self._h, int(col), int(mode), int(seed) & (2 ** 64 - 1), int(max_keys), int(miss_row)))

    def key_space(self, col):
        """-> (mode, seed, max_keys, n_keys, miss_row) of index column col (fr_ctx_key_space; synchronises the device)."""
        mode, seed, mk, nk, miss = ctypes.c_int(), ctypes.c_uint64(), ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int32()
        _check(lib().fr_ctx_key_space(self._h, int(col), ctypes.byref(mode), ctypes.byref(seed), ctypes.byref(mk), ctypes.byref(nk), ctypes.byref(miss)))
        return mode.value, seed.value, mk.value, nk.value, miss.value

    def put_keys(self, col, keys, rows):
        """fr_ctx_put_keys: upsert the pairs (keys[i] int64, rows[i] int32) into the map of MAPPED column col; synchronous, legal beside workers in
        flight.  A pair that cannot be applied (a key of -1, an illegal row, a new key for a full map) raises FleetRecError(FR_ERR_INDEX_RANGE); every
        other pair is applied."""
        k = np.ascontiguousarray(keys, dtype=np.int64).reshape(-1)
        r = np.ascontiguousarray(rows, dtype=np.int32).reshape(-1)
        if k.size != r.size:
            raise FleetRecError(FR_ERR_INVALID, "%d keys, %d rows" % (k.size, r.size))
        _check(lib().fr_ctx_put_keys(self._h, int(col), int(k.size), k.ctypes.data, r.ctypes.data))

    def erase_keys(self, col, keys):
        """fr_ctx_erase_keys: the row of every PRESENT key (int64) of MAPPED column col becomes the column's miss_row; an absent key writes nothing.
        Synchronous, legal beside workers in flight.  A key of -1 raises FleetRecError(FR_ERR_INDEX_RANGE); every other key is applied."""
        k = np.ascontiguousarray(keys, dtype=np.int64).reshape(-1)
        _check(lib().fr_ctx_erase_keys(self._h, int(col), int(k.size), k.ctypes.data))

    def key_space_stats(self, col):
        """-> (slots, occupied, live, probe_sum) of the map of MAPPED column col (fr_ctx_key_space_stats; synchronises the device):
        1 + probe_sum / occupied is the mean number of probes of a present key."""
        s, o, l, p = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        _check(lib().fr_ctx_key_space_stats(self._h, int(col), ctypes.byref(s), ctypes.byref(o), ctypes.byref(l), ctypes.byref(p)))
        return s.value, o.value, l.value, p.value

    def export_keys(self, col):
        """-> (keys int64 [live], rows int32 [live]): the live pairs of the map of MAPPED column col, in unspecified order (fr_ctx_export_keys: the
        size query, then the export; synchronises the device)."""
        n = ctypes.c_int64()
        rc = lib().fr_ctx_export_keys(self._h, int(col), 0, None, None, ctypes.byref(n))
        if rc != FR_OK and not (rc == FR_ERR_INVALID and n.value > 0):
            _check(rc)
        k, r = np.empty(n.value, np.int64), np.empty(n.value, np.int32)
        if n.value:
            _check(lib().fr_ctx_export_keys(self._h, int(col), int(n.value), k.ctypes.data, r.ctypes.data, ctypes.byref(n)))
        return k, r

    def rebuild_key_space(self, col, seed, max_keys):
        """fr_ctx_rebuild_key_space: replace the map of MAPPED column col by one for max_keys keys under `seed` that holds exactly its live pairs
        (dead slots are dropped); on the device, synchronous; no worker of the context may have work in flight."""
        _check(lib().fr_ctx_rebuild_key_space(self._h, int(col), int(seed) & (2 ** 64 - 1), int(max_keys)))

    def set_row_pool(self, col, first_row, n_rows):
        """fr_ctx_set_row_pool: the rows [first_row, first_row + n_rows) of MAPPED column col become its row pool, which admit_keys hands out and
        erase_keys takes back; the free set is derived from the map as it stands (a pool row held by a live key is taken).  n_rows = 0 drops the pool."""
        _check(lib().fr_ctx_set_row_pool(self._h, int(col), int(first_row), int(n_rows)))

    def row_pool(self, col):
        """-> (first_row, n_rows, free_rows) of the row pool of index column col; n_rows = 0: no pool (fr_ctx_row_pool; synchronises the device)."""
        first, n, free = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int64()
        _check(lib().fr_ctx_row_pool(self._h, int(col), ctypes.byref(first), ctypes.byref(n), ctypes.byref(free)))
        return first.value, n.value, free.value

    def admit_keys(self, col, keys):
        """fr_ctx_admit_keys: -> int32 rows, one per key (int64) of MAPPED column col: a live key's own row, for an absent or dead key a free row of
        the column's pool, now its row.  Synchronous, legal beside workers in flight.  A key that cannot be applied (-1, no free row, a new key for a
        full map) raises FleetRecError(FR_ERR_INDEX_RANGE) after every other key was applied; the rows are then in the exception's `rows`."""
        k = np.ascontiguousarray(keys, dtype=np.int64).reshape(-1)
        rows = np.empty(k.size, np.int32)
        try:
            _check(lib().fr_ctx_admit_keys(self._h, int(col), int(k.size), k.ctypes.data, rows.ctypes.data))
        except FleetRecError as e:
            e.rows = rows
            raise
        return rows

    def synchronize(self):
        _check(lib().fr_device_synchronize(self._h))

    def buffer(self, nbytes):
        return DeviceBuffer(self, nbytes)


class Worker:
    """One stream + staging buffers = one thread_consume() of the reference server."""

    def __init__(self, ctx, max_batch):
        self.ctx, self.max_batch = ctx, max_batch
        h = ctypes.c_void_p()
        _check(lib().fr_worker_create(ctx._h, max_batch, ctypes.byref(h)))
        self._h = h
        m = ctx.model
        self.idx = np.ctypeslib.as_array(lib().fr_worker_idx_ptr(h), shape=(max_batch, m.idx_cols))
        self.score = np.ctypeslib.as_array(lib().fr_worker_score_ptr(h), shape=(max_batch,))
        self.dense = (np.ctypeslib.as_array(lib().fr_worker_dense_ptr(h), shape=(max_batch, m.dense_len))
                      if m.dense_len else None)
        self._pool_cap = max(m.idx_cols, ctx.pooled_index_cols)   # int32 columns per item the pinned index buffer holds
        self._pool_w_cap = ctx.pooled_index_cols                  # floats per item the pinned weight buffer holds (0: there is none)
        self._req_caps = (1, 1)                                   # words per request the pinned request index / weight buffers hold (request_buffers)
        req_ptr = getattr(lib(), "fr_worker_request_idx_ptr", None)   # (None: an FR_LIB build from before the request form)
        if req_ptr is not None and req_ptr(h):
            rp = ctx.request_words(REQ_POOLED)[0] if ctx.pooled_index_cols > 0 else 0
            self._req_caps = (max(ctx.request_words(REQ_ONE_HOT)[0], rp, 1), max(rp, 1))

    def close(self):
        if self._h:
            lib().fr_worker_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def submit(self, batch):
        _check(lib().fr_worker_submit(self._h, batch))

    def sync(self):
        _check(lib().fr_worker_sync(self._h))

    def calibrate_fp8(self, idx, dense=None):
        """fp8 chain: run this batch through the fp32 chain and derive the activation exponents from the observed maxima."""
        idx = np.asarray(idx, dtype=np.int32).reshape(len(idx), -1)
        B = idx.shape[0]
        self.idx[:B] = idx
        if self.dense is not None:
            self.dense[:B] = np.asarray(dense, dtype=np.float32).reshape(B, -1)
        _check(lib().fr_worker_calibrate_fp8(self._h, B))

    def infer(self, idx, dense=None):
        """Host-buffer path: idx int32 [B][idx_cols] (+ dense float32 [B][dense_len]) -> scores float32 [B]."""
        idx = np.asarray(idx, dtype=np.int32).reshape(len(idx), -1)
        B = idx.shape[0]
        self.idx[:B] = idx
        if self.dense is not None:
            self.dense[:B] = np.asarray(dense, dtype=np.float32).reshape(B, -1)
        self.submit(B)
        self.sync()
        return self.score[:B].copy()

    @staticmethod
    def _ptr(x):
        if x is None:
            return None
        return x.ptr if isinstance(x, DeviceBuffer) else ctypes.c_void_p(x)

    def infer_sharded(self, comm, idx, dense=None):
        """The sharded hot-loop body (collective): this rank's worker receives the WHOLE request batch; -> all `batch` scores."""
        idx = np.asarray(idx, dtype=np.int32).reshape(len(idx), -1)
        B = idx.shape[0]
        self.idx[:B] = idx
        if self.dense is not None:
            self.dense[:B] = np.asarray(dense, dtype=np.float32).reshape(B, -1)
        _check(lib().fr_worker_submit_sharded(self._h, comm._h, B))
        self.sync()
        return self.score[:B].copy()

    def submit_sharded(self, comm, batch):
        """fr_worker_submit_sharded on the rows already in self.idx / self.dense (asynchronous; follow with sync())."""
        _check(lib().fr_worker_submit_sharded(self._h, comm._h, int(batch)))

    def inject_fc_failure(self, steps):
        """fleetrec_diag.h test hook: this worker's next `steps` sharded steps report a failed FC chain (failure protocol, kind (2))."""
        _check(lib().fr_worker_inject_fc_failure(self._h, int(steps)))

    def calibrate_fp8_sharded(self, comm, idx, dense=None):
        idx = np.asarray(idx, dtype=np.int32).reshape(len(idx), -1)
        B = idx.shape[0]
        self.idx[:B] = idx
        if self.dense is not None:
            self.dense[:B] = np.asarray(dense, dtype=np.float32).reshape(B, -1)
        _check(lib().fr_worker_calibrate_fp8_sharded(self._h, comm._h, B))

    # pooled lookups on sharded contexts (Context(..., hots=...)) ------------------------------------
    def gather_slices_pooled(self, batch, d_idx, d_dense, d_slice, transport, weights=None):
        """fr_worker_gather_slices_pooled: the pooled slice [batch][slice_padded] in the transport type (asynchronous; follow with sync())."""
        _check(lib().fr_worker_gather_slices_pooled(self._h, batch, self._ptr(d_idx), self._ptr(weights), self._ptr(d_dense), self._ptr(d_slice), transport))

    def gather_slices_pooled_csr(self, batch, d_offsets, d_indices, nnz, d_dense, d_slice, transport, weights=None):
        """fr_worker_gather_slices_pooled_csr: the same from the offsets form."""
        _check(lib().fr_worker_gather_slices_pooled_csr(self._h, batch, self._ptr(d_offsets), self._ptr(d_indices), int(nnz), self._ptr(weights), self._ptr(d_dense),
                                                        self._ptr(d_slice), transport))

    def load_pooled(self, idx, dense=None, weights=None):
        """The padded host form of a pooled batch into the pinned buffers: idx int32 [B][P] (+ dense, + weights float32 [B][P]); -> B."""
        idx = self._pooled_rows(idx)
        B, P = idx.shape
        if P > self._pool_cap or (weights is not None and P > self._pool_w_cap):
            raise FleetRecError(FR_ERR_STATE, "the worker's index buffer holds %d columns per item, pooled rows have %d: create the worker "
                                "after Context.set_pooling" % (self._pool_cap, P))
        if B > self.max_batch:
            raise FleetRecError(FR_ERR_INVALID, "batch %d exceeds the worker's max_batch %d" % (B, self.max_batch))
        np.ctypeslib.as_array(lib().fr_worker_idx_ptr(self._h), shape=(B, P))[:] = idx
        if weights is not None:
            np.ctypeslib.as_array(lib().fr_worker_pool_weights_ptr(self._h), shape=(B, P))[:] = self._pooled_weights(weights, idx)
        if self.dense is not None:
            self.dense[:B] = np.asarray(dense, dtype=np.float32).reshape(B, -1)
        return B

    def load_pooled_csr(self, offsets, indices, dense=None, weights=None):
        """The offsets host form of a pooled batch into the pinned buffers (offsets int32 [B * C + 1], indices int32 [nnz], weights float32 [nnz]); -> B."""
        B, off, ind, w = self._csr_arrays(offsets, indices, weights)
        if self.pool_offsets is None or (w is not None and self.pool_weights is None):
            raise FleetRecError(FR_ERR_STATE, "the worker has no offsets buffer: create the worker after Context.set_pooling")
        if B > self.max_batch:
            raise FleetRecError(FR_ERR_INVALID, "batch %d exceeds the worker's max_batch %d" % (B, self.max_batch))
        if ind.size > self.max_batch * self._pool_cap:
            raise FleetRecError(FR_ERR_INVALID, "%d indices exceed the worker's index buffer (%d x %d)" % (ind.size, self.max_batch, self._pool_cap))
        self.pool_offsets[:off.size] = off
        np.ctypeslib.as_array(lib().fr_worker_idx_ptr(self._h), shape=(self.max_batch * self._pool_cap,))[:ind.size] = ind
        if w is not None:
            self.pool_weights.reshape(-1)[:w.size] = w
        if self.dense is not None:
            self.dense[:B] = np.asarray(dense, dtype=np.float32).reshape(B, -1)
        return B

    def submit_sharded_pooled(self, comm, batch, weighted=False):
        """fr_worker_submit_sharded_pooled on the pooled rows already in the pinned buffers (load_pooled; asynchronous, follow with sync())."""
        _check(lib().fr_worker_submit_sharded_pooled(self._h, comm._h, int(batch), 1 if weighted else 0))

    def submit_sharded_pooled_csr(self, comm, batch, weighted=False):
        """fr_worker_submit_sharded_pooled_csr on the offsets-form batch already in the pinned buffers (load_pooled_csr)."""
        _check(lib().fr_worker_submit_sharded_pooled_csr(self._h, comm._h, int(batch), 1 if weighted else 0))

    def calibrate_fp8_sharded_pooled(self, comm, idx, dense=None, weights=None):
        """fr_worker_calibrate_fp8_sharded_pooled (a synchronous collective: one thread per rank on the host exchange)."""
        B = self.load_pooled(idx, dense, weights)
        _check(lib().fr_worker_calibrate_fp8_sharded_pooled(self._h, comm._h, B, 1 if weights is not None else 0))

    def submit_device(self, batch, d_idx, d_dense, d_scores):
        _check(lib().fr_worker_submit_device(self._h, batch, self._ptr(d_idx), self._ptr(d_dense), self._ptr(d_scores)))

    def push_host(self, idx, dense, scores_out):
        """Host-fed streaming push: idx int32 [B][idx_cols] (+ dense float32 [B][dense_len]); scores_out: a float32 numpy array of
        at least B elements that stays alive until sync() -- it receives the scores."""
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        B = idx.shape[0]
        d = None if dense is None else np.ascontiguousarray(dense, dtype=np.float32)
        assert scores_out.dtype == np.float32 and scores_out.flags["C_CONTIGUOUS"] and scores_out.size >= B
        _check(lib().fr_worker_push_host(self._h, B, idx.ctypes.data_as(ctypes.c_void_p), None if d is None else d.ctypes.data_as(ctypes.c_void_p),
                                         scores_out.ctypes.data_as(ctypes.c_void_p)))

    def stage_acquire(self, batch):
        """Zero-copy host-fed push, step 1: numpy views (idx int32 [batch][idx_cols], dense float32 [batch][dense_len] or None) of the
        worker's pinned staging slot for the NEXT pushed batch; fill them, then push_staged()."""
        pi, pd = ctypes.c_void_p(), ctypes.c_void_p()
        _check(lib().fr_worker_stage_acquire(self._h, batch, ctypes.byref(pi), ctypes.byref(pd)))
        m = self.ctx.model
        idx = np.ctypeslib.as_array(ctypes.cast(pi, ctypes.POINTER(ctypes.c_int32)), shape=(batch, m.idx_cols))
        dense = np.ctypeslib.as_array(ctypes.cast(pd, ctypes.POINTER(ctypes.c_float)), shape=(batch, m.dense_len)) if (m.dense_len and pd.value) else None
        return idx, dense

    def push_staged(self, batch, scores_out):
        """Step 2: queue the batch written into the acquired slot; scores_out as for push_host()."""
        assert scores_out.dtype == np.float32 and scores_out.flags["C_CONTIGUOUS"] and scores_out.size >= batch
        _check(lib().fr_worker_push_staged(self._h, batch, scores_out.ctypes.data_as(ctypes.c_void_p)))

    def flush(self):
        """Launch what is queued on the worker now, without waiting (fr_worker_flush)."""
        _check(lib().fr_worker_flush(self._h))

    def host_pending(self):
        """-> (queued, in_flight, blocks_in_flight): host-fed batches in the block being filled / launched and not delivered yet / launched blocks."""
        q, f, nb = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        _check(lib().fr_worker_host_pending(self._h, ctypes.byref(q), ctypes.byref(f), ctypes.byref(nb)))
        return q.value, f.value, nb.value

    def host_poll(self):
        """Deliver the scores of finished host-fed blocks (no waiting); -> host-fed batches delivered so far, in push order."""
        n = ctypes.c_longlong()
        _check(lib().fr_worker_host_poll(self._h, ctypes.byref(n)))
        return n.value

    def update_rows(self, table, n, d_row_ids, d_rows):
        """fr_worker_update_rows: n listed rows of one table from DeviceBuffers (int32 [n] ids, float32 [n][dim] rows), asynchronous on the
        worker's stream, ordered against its batches; both buffers stay untouched until sync()."""
        _check(lib().fr_worker_update_rows(self._h, table, int(n), self._ptr(d_row_ids), self._ptr(d_rows)))

    def push_device(self, batch, d_idx, d_dense, d_scores):
        _check(lib().fr_worker_push_device(self._h, batch, self._ptr(d_idx), self._ptr(d_dense), self._ptr(d_scores)))

    def make_push_list(self, batches, d_idx, d_dense, d_scores):
        """Pre-built argument arrays for push_device_list: batches [n] ints, d_idx / d_scores [n] DeviceBuffers (or pointers), d_dense [n] or None."""
        n = len(batches)
        vp = ctypes.c_void_p
        arr = lambda xs: (vp * n)(*[self._ptr(x) for x in xs])
        return (n, (ctypes.c_int * n)(*[int(b) for b in batches]), arr(d_idx), arr(d_dense) if d_dense is not None else None, arr(d_scores),
                (d_idx, d_dense, d_scores))   # (the buffers stay referenced as long as the list does)

    def push_device_list(self, plist):
        """n consecutive push_device calls in one native call (fr_worker_push_device_list); plist from make_push_list."""
        _check(lib().fr_worker_push_device_list(self._h, plist[0], plist[1], plist[2], plist[3], plist[4]))

    def gather_only(self, batch, d_idx, d_dense, d_records):
        _check(lib().fr_worker_gather_only(self._h, batch, self._ptr(d_idx), self._ptr(d_dense), self._ptr(d_records)))

    def fc_only(self, batch, d_records, d_scores):
        _check(lib().fr_worker_fc_only(self._h, batch, self._ptr(d_records), self._ptr(d_scores)))

    def fc_layer_only(self, batch, layer):
        _check(lib().fr_worker_fc_layer_only(self._h, batch, layer))

    def fc_layer_repeat(self, batch, layer, n):
        """n launches of one layer back to back from one native call (fr_worker_fc_layer_repeat)."""
        _check(lib().fr_worker_fc_layer_repeat(self._h, batch, layer, n))

    def last_kernel(self):
        """The kernel (instantiation included) of this worker's most recent fused / layer / gather launch (fr_worker_last_kernel)."""
        return (lib().fr_worker_last_kernel(self._h) or b"").decode()

    def fc_from_slices(self, batch_total, item0, n_items, d_gathered, d_scores):
        _check(lib().fr_worker_fc_from_slices(self._h, batch_total, item0, n_items, self._ptr(d_gathered), self._ptr(d_scores)))

    def stream_ptr(self):
        """The worker's hipStream_t as an integer (torch.cuda.ExternalStream(ptr) orders torch streams against it)."""
        return lib().fr_worker_stream(self._h)

    def gather_slices(self, batch, d_idx, d_dense, d_slice, transport):
        _check(lib().fr_worker_gather_slices(self._h, batch, self._ptr(d_idx), self._ptr(d_dense), self._ptr(d_slice), transport))

    def fc_from_slices_lp(self, batch_total, item0, n_items, d_gathered, transport, d_scores):
        _check(lib().fr_worker_fc_from_slices_lp(self._h, batch_total, item0, n_items, self._ptr(d_gathered), transport, self._ptr(d_scores)))

    def calibrate_fp8_slices(self, batch_total, item0, n_items, d_gathered):
        _check(lib().fr_worker_calibrate_fp8_slices(self._h, batch_total, item0, n_items, self._ptr(d_gathered)))

    def records_dptr(self):
        return lib().fr_worker_records_dptr(self._h)

    def features(self, batch, bf16=False, fp8=False):
        """Feature-major activations of the last submit(), un-packed from the device's q4 layout Xq[k/4][m][k%4]
        -> uint32 [record_len][batch] (debug/parity hook for the pipeline's own gather stage)."""
        ld_max = ctypes.c_int()
        p = lib().fr_worker_features_dptr(self._h, ctypes.byref(ld_max))
        K = self.ctx.model.record_len
        ld = (batch + 31) // 32 * 32
        if fp8:  # q16 layout Xf[k/16][m][k%16] of e4m3 bytes, K zero-padded to a multiple of 64 -> uint8 [KP][batch]
            KP = (K + 63) // 64 * 64
            out = np.empty(KP * ld, dtype=np.uint8)
            _check(lib().fr_memcpy_d2h(self.ctx._h, out.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(p), out.nbytes))
            return out.reshape(KP // 16, ld, 16).transpose(0, 2, 1).reshape(KP, ld)[:, :batch]
        if bf16:  # q8 layout Xh[k/8][m][k%8] of bf16 -> uint16 [record_len][batch]
            out = np.empty(K * ld, dtype=np.uint16)
            _check(lib().fr_memcpy_d2h(self.ctx._h, out.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(p), out.nbytes))
            return out.reshape(K // 8, ld, 8).transpose(0, 2, 1).reshape(K, ld)[:, :batch]
        out = np.empty(K * ld, dtype=np.uint32)
        _check(lib().fr_memcpy_d2h(self.ctx._h, out.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(p), out.nbytes))
        return out.reshape(K // 4, ld, 4).transpose(0, 2, 1).reshape(K, ld)[:, :batch]

    def timer_start(self):
        _check(lib().fr_worker_timer_start(self._h))

    def timer_stop_ms(self):
        ms = ctypes.c_float()
        _check(lib().fr_worker_timer_stop_ms(self._h, ctypes.byref(ms)))
        return ms.value

    # multi-hot pooled lookups (Context.set_pooling) ------------------------------------------------
    def gather_pooled(self, batch, d_idx, d_dense, d_records, weights=None):
        """d_idx int32 [batch][ctx.pooled_index_cols] -> fp32 records in the model's layout (asynchronous; follow with sync()).
        weights: device float32 [batch][ctx.pooled_index_cols], the weight of every slot (fr_worker_gather_pooled_weighted)."""
        if weights is None:
            _check(lib().fr_worker_gather_pooled(self._h, batch, self._ptr(d_idx), self._ptr(d_dense), self._ptr(d_records)))
        else:
            _check(lib().fr_worker_gather_pooled_weighted(self._h, batch, self._ptr(d_idx), self._ptr(weights), self._ptr(d_dense), self._ptr(d_records)))

    def submit_pooled_device(self, batch, d_idx, d_dense, d_scores, weights=None):
        if weights is None:
            _check(lib().fr_worker_submit_pooled_device(self._h, batch, self._ptr(d_idx), self._ptr(d_dense), self._ptr(d_scores)))
        else:
            _check(lib().fr_worker_submit_pooled_weighted_device(self._h, batch, self._ptr(d_idx), self._ptr(weights), self._ptr(d_dense), self._ptr(d_scores)))

    def submit_pooled(self, batch, weighted=False):
        """fr_worker_submit_pooled on the pooled rows already in the pinned index buffer (asynchronous; follow with sync());
        weighted: fr_worker_submit_pooled_weighted, with the weights already in pool_weights."""
        _check((lib().fr_worker_submit_pooled_weighted if weighted else lib().fr_worker_submit_pooled)(self._h, int(batch)))

    @property
    def pool_weights(self):
        """float32 [max_batch][P] view of the pinned weight buffer (fr_worker_pool_weights_ptr); None on a worker created before
        Context.set_pooling."""
        p = lib().fr_worker_pool_weights_ptr(self._h)
        if not p or self._pool_w_cap <= 0:
            return None
        return np.ctypeslib.as_array(p, shape=(self.max_batch, self._pool_w_cap))

    def _pooled_rows(self, idx):
        P = self.ctx.pooled_index_cols
        if P <= 0:
            raise FleetRecError(FR_ERR_STATE, "no pooling is set on the context: call Context.set_pooling first")
        idx = np.ascontiguousarray(np.asarray(idx, dtype=np.int32).reshape(len(idx), -1))
        if idx.shape[1] != P:
            raise FleetRecError(FR_ERR_INVALID, "pooled index rows have %d columns, the context's pooling needs %d" % (idx.shape[1], P))
        return idx

    @staticmethod
    def _pooled_weights(weights, idx):
        w = np.ascontiguousarray(np.asarray(weights, dtype=np.float32).reshape(len(weights), -1))
        if w.shape != idx.shape:
            raise FleetRecError(FR_ERR_INVALID, "per-sample weights are %s, the pooled index rows %s" % (w.shape, idx.shape))
        return w

    def infer_pooled(self, idx, dense=None, weights=None):
        """Host-buffer path of the pooled lookup: idx int32 [B][pooled_index_cols] (-1 = empty slot) (+ dense) -> scores float32 [B].
        weights: float32 [B][pooled_index_cols], the weight of every slot (all-SUM contexts only).
        The worker must have been created after Context.set_pooling (its pinned index and weight buffers are sized then)."""
        B = self.load_pooled(idx, dense, weights)
        self.submit_pooled(B, weighted=weights is not None)
        self.sync()
        return self.score[:B].copy()

    def gather_pooled_records(self, idx, dense=None, weights=None):
        """-> uint32 [flat B*K] record buffer in the model's layout: the pooled records of idx int32 [B][pooled_index_cols]
        (weights: float32 of the same shape, the weight of every slot)."""
        idx = self._pooled_rows(idx)
        n = len(idx) * self.ctx.model.record_len
        with self._on_device(n, dense, idx=idx, w=self._pooled_weights(weights, idx) if weights is not None else None) as d:
            self.gather_pooled(len(idx), d["idx"], d["dense"], d["rec"], weights=d["w"])
            self.sync()
            return d["rec"].download(np.uint32, n)

    @contextlib.contextmanager
    def _on_device(self, n_rec, dense, **arrays):
        """-> {name: device copy of the host array (None stays None)} + "dense" (the dense features, None without) + "rec" (room for n_rec record
        words); every buffer is freed on the way out, also when an allocation fails part-way"""
        ctx, d = self.ctx, {}
        try:
            for name, a in arrays.items():
                d[name] = DeviceBuffer.from_numpy(ctx, a) if a is not None else None
            d["dense"] = DeviceBuffer.from_numpy(ctx, np.asarray(dense, dtype=np.float32)) if ctx.model.dense_len else None
            d["rec"] = DeviceBuffer(ctx, n_rec * 4)
            yield d
        finally:
            for b in d.values():
                if b is not None:
                    b.free()

    # the offsets (CSR) form of the pooled lookups: bag (b, c) = indices[offsets[b * C + c] : offsets[b * C + c + 1]], C = model.idx_cols ----
    def gather_pooled_csr(self, batch, d_offsets, d_indices, nnz, d_dense, d_records, weights=None):
        """d_offsets int32 [batch * C + 1], d_indices int32 [nnz] (None when nnz == 0), weights: device float32 [nnz] or None -> fp32 records in
        the model's layout (fr_worker_gather_pooled_csr; asynchronous, follow with sync())."""
        _check(lib().fr_worker_gather_pooled_csr(self._h, batch, self._ptr(d_offsets), self._ptr(d_indices), int(nnz), self._ptr(weights), self._ptr(d_dense),
                                                 self._ptr(d_records)))

    def submit_pooled_csr_device(self, batch, d_offsets, d_indices, nnz, d_dense, d_scores, weights=None):
        _check(lib().fr_worker_submit_pooled_csr_device(self._h, batch, self._ptr(d_offsets), self._ptr(d_indices), int(nnz), self._ptr(weights), self._ptr(d_dense),
                                                        self._ptr(d_scores)))

    # streaming pushes of pooled batches: nothing waits, sync() is the completion point; every buffer stays valid (scores distinct) until then ----
    def push_pooled_device(self, batch, d_idx, d_dense, d_scores, weights=None):
        """fr_worker_push_pooled_device: push_device for a pooled batch (d_idx int32 [batch][ctx.pooled_index_cols]; weights: device float32 of
        the same shape, or None for the unweighted fold)."""
        _check(lib().fr_worker_push_pooled_device(self._h, batch, self._ptr(d_idx), self._ptr(weights), self._ptr(d_dense), self._ptr(d_scores)))

    def push_pooled_csr_device(self, batch, d_offsets, d_indices, nnz, d_dense, d_scores, weights=None):
        """fr_worker_push_pooled_csr_device: the offsets form (arguments as submit_pooled_csr_device)."""
        _check(lib().fr_worker_push_pooled_csr_device(self._h, batch, self._ptr(d_offsets), self._ptr(d_indices), int(nnz), self._ptr(weights), self._ptr(d_dense),
                                                      self._ptr(d_scores)))

    def make_pooled_push_list(self, batches, d_idx, d_dense, d_scores, weights=None):
        """Pre-built argument arrays for push_pooled_device_list: batches [n] ints, d_idx / d_scores [n] DeviceBuffers (or pointers), d_dense [n] or
        None, weights [n] (entries may be None) or None."""
        n = len(batches)
        vp = ctypes.c_void_p
        arr = lambda xs: (vp * n)(*[self._ptr(x) for x in xs])
        return (n, (ctypes.c_int * n)(*[int(b) for b in batches]), arr(d_idx), arr(weights) if weights is not None else None,
                arr(d_dense) if d_dense is not None else None, arr(d_scores), (d_idx, weights, d_dense, d_scores))   # (the buffers stay referenced)

    def push_pooled_device_list(self, plist):
        """n consecutive push_pooled_device calls in one native call (fr_worker_push_pooled_device_list); plist from make_pooled_push_list."""
        _check(lib().fr_worker_push_pooled_device_list(self._h, plist[0], plist[1], plist[2], plist[3], plist[4], plist[5]))

    def submit_pooled_csr(self, batch, weighted=False):
        """fr_worker_submit_pooled_csr on the offsets in pool_offsets, the flat entries in the pinned index buffer and (weighted) the flat weights
        in the pinned weight buffer (asynchronous; follow with sync())."""
        _check(lib().fr_worker_submit_pooled_csr(self._h, int(batch), 1 if weighted else 0))

    @property
    def pool_offsets(self):
        """int32 [max_batch * C + 1] view of the pinned offsets buffer (fr_worker_pool_offsets_ptr); None on a worker created before
        Context.set_pooling."""
        p = lib().fr_worker_pool_offsets_ptr(self._h)
        if not p:
            return None
        return np.ctypeslib.as_array(p, shape=(self.max_batch * self.ctx.model.idx_cols + 1,))

    def _csr_arrays(self, offsets, indices, weights):
        if self.ctx.pooled_index_cols <= 0:
            raise FleetRecError(FR_ERR_STATE, "no pooling is set on the context: call Context.set_pooling first")
        C = self.ctx.model.idx_cols
        off = np.ascontiguousarray(np.asarray(offsets, dtype=np.int32).reshape(-1))
        if off.size < 1 or (off.size - 1) % C:
            raise FleetRecError(FR_ERR_INVALID, "%d offsets are not batch x %d index columns + 1" % (off.size, C))
        ind = np.ascontiguousarray(np.asarray(indices, dtype=np.int32).reshape(-1))
        w = None
        if weights is not None:
            w = np.ascontiguousarray(np.asarray(weights, dtype=np.float32).reshape(-1))
            if w.size != ind.size:
                raise FleetRecError(FR_ERR_INVALID, "%d per-sample weights for %d indices" % (w.size, ind.size))
        return (off.size - 1) // C, off, ind, w

    def infer_pooled_csr(self, offsets, indices, dense=None, weights=None):
        """Host-buffer path of the offsets-form pooled lookup: offsets int32 [B * C + 1], indices int32 [nnz] (-1 = empty slot), weights float32
        [nnz] or None (+ dense) -> scores float32 [B].  The worker must have been created after Context.set_pooling."""
        B = self.load_pooled_csr(offsets, indices, dense, weights)
        self.submit_pooled_csr(B, weighted=weights is not None)
        self.sync()
        return self.score[:B].copy()

    def gather_pooled_csr_records(self, offsets, indices, dense=None, weights=None):
        """-> uint32 [flat B*K] record buffer in the model's layout: the pooled records of the bags offsets / indices (/ weights) describe."""
        B, off, ind, w = self._csr_arrays(offsets, indices, weights)
        n = B * self.ctx.model.record_len
        with self._on_device(n, dense, off=off, ind=ind if ind.size else None, w=(w if w.size else np.zeros(1, np.float32)) if w is not None else None) as d:
            self.gather_pooled_csr(B, d["off"], d["ind"], ind.size, d["dense"], d["rec"], weights=d["w"])
            self.sync()
            return d["rec"].download(np.uint32, n)

    # segmented top-K ranking of scores (fr_worker_topk_device / fr_worker_topk) ------------------------------------------------
    def topk_device(self, n, d_scores, k, d_top_idx, d_top_scores=None, d_seg_offsets=None, n_seg=1):
        """fr_worker_topk_device: ranks the n device scores in n_seg segments (d_seg_offsets int32 [n_seg + 1]; None: one segment [0, n)) on the
        worker's stream, behind everything submitted or pushed before; d_top_idx int32 [n_seg][k] (positions inside the segment, -1 past its
        length), d_top_scores float32 [n_seg][k] or None.  Asynchronous: sync() is the completion point, the buffers stay valid until then."""
        _check(lib().fr_worker_topk_device(self._h, int(n), self._ptr(d_scores), int(n_seg), self._ptr(d_seg_offsets), int(k), self._ptr(d_top_idx), self._ptr(d_top_scores)))

    def _topk_host(self, B, k, seg_offsets):
        """fr_worker_topk on the host-form batch in flight, then sync() -> (idx int32 [n_seg][k], scores float32 [n_seg][k])"""
        off = None if seg_offsets is None else np.ascontiguousarray(np.asarray(seg_offsets, dtype=np.int32).reshape(-1))
        n_seg = 1 if off is None else off.size - 1
        out_i, out_s = np.empty((max(n_seg, 0), int(k)), np.int32), np.empty((max(n_seg, 0), int(k)), np.float32)
        try:
            _check(lib().fr_worker_topk(self._h, B, n_seg, None if off is None else off.ctypes.data_as(ctypes.c_void_p), int(k),
                                        out_i.ctypes.data_as(ctypes.c_void_p), out_s.ctypes.data_as(ctypes.c_void_p)))
        except FleetRecError:
            try:
                self.sync()   # the batch that was submitted is not left in flight
            except FleetRecError:
                pass
            raise
        self.sync()
        return out_i, out_s

    def infer_topk(self, idx, k, seg_offsets=None, dense=None):
        """infer() with the ranking on the device: idx int32 [B][idx_cols] (+ dense) -> (positions int32 [n_seg][k], scores float32 [n_seg][k]) of the
        batch's scores ranked in the segments seg_offsets int32 [n_seg + 1] describes (None: the whole batch is one segment)."""
        idx = np.asarray(idx, dtype=np.int32).reshape(len(idx), -1)
        B = idx.shape[0]
        self.idx[:B] = idx
        if self.dense is not None:
            self.dense[:B] = np.asarray(dense, dtype=np.float32).reshape(B, -1)
        self.submit(B)
        return self._topk_host(B, k, seg_offsets)

    def infer_pooled_topk(self, idx, k, seg_offsets=None, dense=None, weights=None):
        """infer_pooled() with the ranking on the device (arguments of infer_pooled; k / seg_offsets / result of infer_topk)."""
        B = self.load_pooled(idx, dense, weights)
        self.submit_pooled(B, weighted=weights is not None)
        return self._topk_host(B, k, seg_offsets)

    def infer_pooled_csr_topk(self, offsets, indices, k, seg_offsets=None, dense=None, weights=None):
        """infer_pooled_csr() with the ranking on the device (arguments of infer_pooled_csr; k / seg_offsets / result of infer_topk)."""
        B = self.load_pooled_csr(offsets, indices, dense, weights)
        self.submit_pooled_csr(B, weighted=weights is not None)
        return self._topk_host(B, k, seg_offsets)

    # request-form batches (Context.set_request_columns): request rows + candidate rows + segment offsets, expanded on the device ----------------
    def expand_requests_device(self, batch, n_req, d_req, d_cand, d_out, form, d_seg_offsets=None):
        """fr_worker_expand_requests_device: d_req [n_req][request words] + d_cand [batch][candidate words] (None for REQ_DENSE) -> d_out
        [batch][row words] of the form, 32-bit bit copies; d_seg_offsets int32 [n_req + 1] (None: n_req equal requests).  Asynchronous on the
        worker's stream: a following gather / submit / push on this worker with d_out as its rows reads the expanded rows; sync() completes it."""
        _check(lib().fr_worker_expand_requests_device(self._h, int(batch), int(n_req), self._ptr(d_seg_offsets), self._ptr(d_req), self._ptr(d_cand), int(form),
                                                      self._ptr(d_out)))

    def request_buffers(self):
        """-> (idx int32, weights float32 or None, dense float32 or None, offsets int32): flat numpy views of the four pinned request buffers
        (fr_worker_request_*_ptr), max_batch x the words per request the worker was created for (offsets: max_batch + 1); request rows are packed
        [n_req][request words of the form].  (None, None, None, None) on a worker created before Context.set_request_columns."""
        L, B = lib(), self.max_batch
        p = L.fr_worker_request_idx_ptr(self._h)
        if not p:
            return None, None, None, None
        ri, rw = self._req_caps   # words per request the buffers were sized for when the worker was created
        pw, pd = L.fr_worker_request_weights_ptr(self._h), L.fr_worker_request_dense_ptr(self._h)
        return (np.ctypeslib.as_array(p, shape=(B * ri,)),
                np.ctypeslib.as_array(pw, shape=(B * rw,)) if pw else None,
                np.ctypeslib.as_array(pd, shape=(B * self.ctx.model.dense_len,)) if pd else None,
                np.ctypeslib.as_array(L.fr_worker_request_offsets_ptr(self._h), shape=(B + 1,)))

    def submit_requests(self, batch, n_req, pooled=0):
        """fr_worker_submit_requests on what the pinned buffers hold (candidate side: the index / pool-weight / dense buffers; request side:
        request_buffers()); pooled: 0 one-hot, 1 pooled, 2 pooled weighted.  Asynchronous; follow with sync()."""
        _check(lib().fr_worker_submit_requests(self._h, int(batch), int(n_req), int(pooled)))

    def _load_requests(self, req_idx, cand_idx, seg_offsets, req_dense, dense, req_weights, weights, pooled):
        """fills the pinned buffers of a request-form host call -> (batch, n_req, pooled, offsets)"""
        ctx = self.ctx
        off = np.ascontiguousarray(np.asarray(seg_offsets, dtype=np.int32).reshape(-1))
        n_req = off.size - 1
        weighted = weights is not None or req_weights is not None
        cand = np.asarray(cand_idx, dtype=np.int32)
        B = len(cand)
        if pooled is None:   # the pooled form on a context whose pooling is set
            pooled = 1 if ctx.pooled_index_cols > 0 or weighted else 0
        pooled = 2 if pooled and weighted else int(pooled)
        rs, rc, _ = ctx.request_words(REQ_POOLED if pooled else REQ_ONE_HOT)
        b_idx, b_w, b_dense, b_off = self.request_buffers()
        if b_idx is None:
            raise FleetRecError(FR_ERR_STATE, "the worker has no request buffers: create the worker after Context.set_request_columns")
        if B > self.max_batch or n_req < 1 or n_req > self.max_batch:
            raise FleetRecError(FR_ERR_INVALID, "batch %d / %d requests exceed the worker's max_batch %d" % (B, n_req, self.max_batch))
        req = np.asarray(req_idx, dtype=np.int32).reshape(-1) if rs else np.zeros(0, np.int32)
        cand = cand.reshape(-1)
        if req.size != n_req * rs or cand.size != B * rc or req.size > b_idx.size or cand.size > self.max_batch * self._pool_cap:
            raise FleetRecError(FR_ERR_INVALID, "request rows of %d words and candidate rows of %d words do not match the split's %d x %d and %d x %d" % (req.size, cand.size, n_req, rs, B, rc))
        b_off[:off.size] = off
        b_idx[:req.size] = req
        np.ctypeslib.as_array(lib().fr_worker_idx_ptr(self._h), shape=(self.max_batch * self._pool_cap,))[:cand.size] = cand
        if pooled == 2:
            if b_w is None or self.pool_weights is None:
                raise FleetRecError(FR_ERR_STATE, "the worker has no weight buffers: create the worker after Context.set_pooling")
            b_w[:req.size] = np.asarray(req_weights, dtype=np.float32).reshape(-1) if rs else np.zeros(0, np.float32)
            self.pool_weights.reshape(-1)[:cand.size] = np.asarray(weights, dtype=np.float32).reshape(-1)
        if b_dense is not None:
            b_dense[:n_req * ctx.model.dense_len] = np.asarray(req_dense, dtype=np.float32).reshape(-1)
        elif self.dense is not None:
            self.dense[:B] = np.asarray(dense, dtype=np.float32).reshape(B, -1)
        return B, n_req, pooled, off

    def infer_requests(self, req_idx, cand_idx, seg_offsets, req_dense=None, dense=None, req_weights=None, weights=None, pooled=None):
        """Host-buffer path of a request-form batch: req_idx int32 [n_req][request words], cand_idx int32 [B][candidate words], seg_offsets int32
        [n_req + 1] (+ req_dense [n_req][dense_len] when the dense features are shared, else dense [B][dense_len]) -> scores float32 [B].  On a
        context whose pooling is set the rows are pooled rows (pooled=0 forces the one-hot form); weights / req_weights: float32 of the shapes of
        cand_idx / req_idx, the weight of every slot (all-SUM contexts only)."""
        B, n_req, pooled, _ = self._load_requests(req_idx, cand_idx, seg_offsets, req_dense, dense, req_weights, weights, pooled)
        self.submit_requests(B, n_req, pooled)
        self.sync()
        return self.score[:B].copy()

    def infer_requests_topk(self, req_idx, cand_idx, seg_offsets, k, req_dense=None, dense=None, req_weights=None, weights=None, pooled=None):
        """infer_requests() with the ranking on the device: -> (positions int32 [n_req][k], scores float32 [n_req][k]), every request's candidates
        ranked (fr_worker_topk over the same offsets)."""
        B, n_req, pooled, off = self._load_requests(req_idx, cand_idx, seg_offsets, req_dense, dense, req_weights, weights, pooled)
        self.submit_requests(B, n_req, pooled)
        return self._topk_host(B, k, off)

    # keyed lookups (Context.set_key_space): int64 feature ids resolved to the int32 rows every lookup path takes, on the device ---------------------
    def put_keys(self, col, n, d_keys, d_rows):
        """fr_worker_put_keys: n pairs from device memory (d_keys int64, d_rows int32) into the map of MAPPED column col, asynchronous on the worker's
        stream; both stay valid until sync(), which reports a pair that could not be applied as FR_ERR_INDEX_RANGE."""
        _check(lib().fr_worker_put_keys(self._h, int(col), int(n), self._ptr(d_keys), self._ptr(d_rows)))

    def erase_keys(self, col, n, d_keys):
        """fr_worker_erase_keys: n keys from device memory (d_keys int64); the row of every present one becomes the column's miss_row, asynchronous on
        the worker's stream; a key of -1 is reported by sync()."""
        _check(lib().fr_worker_erase_keys(self._h, int(col), int(n), self._ptr(d_keys)))

    def admit_keys(self, col, n, d_keys, d_rows_out):
        """fr_worker_admit_keys: n keys from device memory (d_keys int64) -> d_rows_out int32: a live key's own row, for an absent or dead key a free
        row of the column's pool, now its row; asynchronous on the worker's stream.  A key that cannot be applied (-1, no free row, a new key for a
        full map) is reported by sync(); d_rows_out is what a following update_rows takes as its row ids."""
        _check(lib().fr_worker_admit_keys(self._h, int(col), int(n), self._ptr(d_keys), self._ptr(d_rows_out)))

    def resolve_keys_device(self, n_rows, d_keys, d_idx_out, rows_kind=KEY_ROWS_FULL, pooled=False):
        """fr_worker_resolve_keys_device: d_keys int64 [n_rows][W] -> d_idx_out int32 [n_rows][W]; W follows rows_kind (KEY_ROWS_FULL: the index or
        pooled row; KEY_ROWS_REQUEST / KEY_ROWS_CANDIDATE: the two sides of the request split) and pooled.  One launch on the worker's stream; a
        following gather / submit / push / expand_requests_device on this worker reads the rows."""
        _check(lib().fr_worker_resolve_keys_device(self._h, int(n_rows), int(rows_kind), int(bool(pooled)), self._ptr(d_keys), self._ptr(d_idx_out)))

    def key_rows(self):
        """-> flat int64 numpy view of the pinned key rows of the keyed host form (fr_worker_key_ptr): max_batch x max(index cols, pooled cols at
        creation); None on a worker created before the context's first non-default key space."""
        p = lib().fr_worker_key_ptr(self._h)
        return np.ctypeslib.as_array(p, shape=(self.max_batch * self._pool_cap,)) if p else None

    def submit_keyed(self, batch, pooled=0):
        """fr_worker_submit_keyed on what key_rows() (and the dense / pool-weight buffers) hold; pooled: 0 one-hot, 1 pooled, 2 pooled weighted.
        Asynchronous; follow with sync()."""
        _check(lib().fr_worker_submit_keyed(self._h, int(batch), int(pooled)))

    def key_misses(self, reset=True):
        """MAPPED lookups of this worker that found no key since the last reset (fr_worker_key_misses; synchronises the worker's stream)."""
        v = ctypes.c_uint64()
        _check(lib().fr_worker_key_misses(self._h, ctypes.byref(v), int(bool(reset))))
        return v.value

    def _load_keys(self, keys, width, dense):
        buf = self.key_rows()
        if buf is None:
            raise FleetRecError(FR_ERR_STATE, "the worker has no key buffer: create the worker after Context.set_key_space")
        if width > self._pool_cap:
            raise FleetRecError(FR_ERR_STATE, "the worker's key buffer holds %d columns per item, the key rows have %d: create the worker after Context.set_pooling" % (self._pool_cap, width))
        k = np.ascontiguousarray(keys, dtype=np.int64)
        B = len(k)
        if B < 1 or B > self.max_batch or k.size != B * width:
            raise FleetRecError(FR_ERR_INVALID, "key rows of shape %s: this call takes [1 .. %d][%d]" % (k.shape, self.max_batch, width))
        buf[:k.size] = k.reshape(-1)
        if dense is not None:
            self.dense[:B] = dense
        return B

    def infer_keyed(self, keys, dense=None):
        """Host-buffer path of a keyed one-hot batch: keys int64 [B][index cols] -> fp32 scores [B]."""
        B = self._load_keys(keys, self.ctx.model.idx_cols, dense)
        self.submit_keyed(B, 0)
        self.sync()
        return self.score[:B].copy()

    def infer_pooled_keyed(self, keys, dense=None, weights=None):
        """Host-buffer path of a keyed pooled batch: keys int64 [B][P] (-1 = empty slot), weights float32 [B][P] or None -> fp32 scores [B]."""
        P = self.ctx.pooled_index_cols
        B = self._load_keys(keys, P, dense)
        if weights is not None:
            pw = self.pool_weights
            if pw is None:
                raise FleetRecError(FR_ERR_STATE, "the worker has no weight buffer: create the worker after Context.set_pooling")
            w = np.ascontiguousarray(weights, dtype=np.float32)
            if w.size != B * P:
                raise FleetRecError(FR_ERR_INVALID, "per-sample weights are %s, the key rows [%d][%d]" % (w.shape, B, P))
            pw.reshape(-1)[:B * P] = w.reshape(-1)
        self.submit_keyed(B, 2 if weights is not None else 1)
        self.sync()
        return self.score[:B].copy()

    # convenience used by the parity tests --------------------------------------------------------
    def gather_records(self, idx, dense=None):
        """-> uint32 [flat B*K] record buffer in the model's layout (bit copy of what the kernel wrote)."""
        ctx, m = self.ctx, self.ctx.model
        idx = np.ascontiguousarray(np.asarray(idx, dtype=np.int32).reshape(len(idx), -1))
        B = idx.shape[0]
        d_idx = DeviceBuffer.from_numpy(ctx, idx)
        d_dense = DeviceBuffer.from_numpy(ctx, np.asarray(dense, dtype=np.float32)) if m.dense_len else None
        info = ctx.shard_info()
        n = B * info["slice_padded"]
        d_rec = DeviceBuffer(ctx, n * 4)
        self.gather_only(B, d_idx, d_dense, d_rec)
        self.sync()
        return d_rec.download(np.uint32, n)

    def fc_scores(self, records_f32):
        ctx = self.ctx
        rec = np.ascontiguousarray(records_f32, dtype=np.float32)
        B = rec.size // ctx.model.record_len
        d_rec = DeviceBuffer.from_numpy(ctx, rec)
        d_sc = DeviceBuffer(ctx, B * 4)
        self.fc_only(B, d_rec, d_sc)
        self.sync()
        return d_sc.download(np.float32, B)


class Comm:
    """One rank's communicator over the shards of a table-sharded model (fr_comm_*): RCCL for GPU contexts, the in-process host
    exchange for CPU contexts (init_all only)."""

    def __init__(self, handle):
        self._h = handle

    @staticmethod
    def unique_id():
        buf = ctypes.create_string_buffer(128)
        _check(lib().fr_comm_unique_id(buf))
        return buf.raw

    @classmethod
    def init_rank(cls, ctx, unique_id):
        h = ctypes.c_void_p()
        _check(lib().fr_comm_init_rank(ctx._h, ctypes.create_string_buffer(unique_id, 128), ctypes.byref(h)))
        return cls(h)

    @classmethod
    def init_all(cls, ctxs):
        n = len(ctxs)
        arr = (ctypes.c_void_p * n)(*[c._h for c in ctxs])
        out = (ctypes.c_void_p * n)()
        _check(lib().fr_comm_init_all(arr, n, out))
        return [cls(ctypes.c_void_p(out[i])) for i in range(n)]

    def set_wait_ms(self, ms):
        """Bound of fr_worker_sync's wait for a sharded step's collectives on this rank (default 60 s)."""
        _check(lib().fr_comm_set_wait_ms(self._h, int(ms)))

    _EXCHANGES = {"allgather": EXCHANGE_ALLGATHER, "alltoall": EXCHANGE_ALLTOALL}

    def set_exchange(self, mode):
        """How this rank's sharded steps exchange the slices: "allgather" (default) or "alltoall" (or EXCHANGE_*); between steps, the same
        mode on every rank of the communicator (fr_comm_set_exchange)."""
        if isinstance(mode, str):
            if mode not in self._EXCHANGES:
                raise FleetRecError(FR_ERR_INVALID, "unknown exchange mode %r (allgather | alltoall)" % mode)
            mode = self._EXCHANGES[mode]
        _check(lib().fr_comm_set_exchange(self._h, int(mode)))

    @property
    def exchange(self):
        """The current exchange mode: EXCHANGE_ALLGATHER or EXCHANGE_ALLTOALL."""
        mode = lib().fr_comm_exchange(self._h)
        if mode < 0:
            _check(mode)
        return mode

    def exchange_bytes(self):
        """-> (received, sent): slice bytes of the last sharded step this rank issued, peers only (fleetrec_diag.h; counted, not measured)."""
        rx, tx = ctypes.c_uint64(), ctypes.c_uint64()
        _check(lib().fr_comm_exchange_bytes(self._h, ctypes.byref(rx), ctypes.byref(tx)))
        return rx.value, tx.value

    def close(self):
        if self._h:
            lib().fr_comm_destroy(self._h)
            self._h = None


class Driver:
    """The reference server's main() + thread_consume() batch loop (without sockets), natively threaded."""

    def __init__(self, ctx, n_threads, depth, max_batch):
        self.ctx, self.n_threads, self.depth = ctx, n_threads, depth
        h = ctypes.c_void_p()
        _check(lib().fr_driver_create(ctx._h, n_threads, depth, max_batch, ctypes.byref(h)))
        self._h = h
        self._pools = {}   # "idx" / "dense" -> (pointer generation, the pool's buffers, their ctypes pointer array): see _pool_array

    def _pool_array(self, which, pool):
        """The ctypes array of a pool's device pointers.  A request stream rotates through ONE pool for its whole life, and marshalling 1024 pointers
        costs as much as a short run: the array of the last pool is kept (with the buffers it was built from, so none of them can be collected and its
        address reused) and handed out again while the list holds the same objects and no DeviceBuffer anywhere was freed or re-pointed since."""
        key = tuple(pool)
        gen = _ptr_generation
        c = self._pools.get(which)
        if c is not None and c[0] == gen and c[1] == key:   # (DeviceBuffer defines no __eq__: the tuples compare by identity)
            return c[2]
        arr = (ctypes.c_void_p * len(key))(*[b.ptr.value for b in key])
        self._pools[which] = (gen, key, arr)
        return arr

    def run_resident(self, batch, total_batches, idx_pool, dense_pool=None):
        """idx_pool / dense_pool: lists of DeviceBuffer.  -> elapsed seconds."""
        n = len(idx_pool)
        ip = self._pool_array("idx", idx_pool)
        dp = self._pool_array("dense", dense_pool) if dense_pool else None
        el = ctypes.c_double()
        _check(lib().fr_driver_run_resident(self._h, batch, total_batches, ip, dp, n, ctypes.byref(el)))
        return el.value

    def score_ring(self, thread, slot, max_batch):
        """-> float32 [ring_len][max_batch]: the scores of the last ring_len batches pushed to worker (thread, slot)."""
        n = ctypes.c_int()
        p = lib().fr_driver_score_ring(self._h, thread, slot, ctypes.byref(n))
        out = np.empty((n.value, max_batch), dtype=np.float32)
        _check(lib().fr_memcpy_d2h(self.ctx._h, out.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(p), out.nbytes))
        return out

    def run_host(self, batch, total_batches, idx_pool_np, dense_pool_np=None, streaming=False):
        """idx_pool_np / dense_pool_np: lists of C-contiguous numpy arrays in host memory.  -> elapsed seconds (PCIe-inclusive).
        streaming=False: submit + sync per batch (the reference's sequence); True: fr_worker_push_host blocks."""
        n = len(idx_pool_np)
        keep = [np.ascontiguousarray(a, dtype=np.int32) for a in idx_pool_np]
        ip = (ctypes.c_void_p * n)(*[a.ctypes.data for a in keep])
        dp = None
        if dense_pool_np:
            keepd = [np.ascontiguousarray(a, dtype=np.float32) for a in dense_pool_np]
            dp = (ctypes.c_void_p * n)(*[a.ctypes.data for a in keepd])
        el = ctypes.c_double()
        _check((lib().fr_driver_run_host_streaming if streaming else lib().fr_driver_run_host)(self._h, batch, total_batches, ip, dp, n, ctypes.byref(el)))
        return el.value

    def host_score_ring(self, thread, slot, max_batch):
        """-> float32 [ring_len][max_batch] (host memory): scores of the last ring_len batches run_host(streaming=True) gave worker (thread, slot)."""
        n = ctypes.c_int()
        p = lib().fr_driver_host_score_ring(self._h, thread, slot, ctypes.byref(n))
        return np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctypes.c_float)), shape=(n.value, max_batch)).copy()

    def close(self):
        if self._h:
            lib().fr_driver_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
