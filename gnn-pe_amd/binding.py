"""ctypes view of the C-ABI in include/gnnpe_hip.h (libgnnpe_hip.so).

This is plumbing for bench.py and the tests: numpy arrays / raw device pointers go in, nothing
torch-typed crosses the boundary.  `load()` raises if the HIP library is missing or cannot be
loaded -- there is deliberately no CPU fallback (the oracle lives in oracle/ and is never
imported from here).
"""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# (GNNPE_LIB_PATH: the A/B scripts under scripts/ point it at the diagnostic build, `make -C gnn-pe_amd DIAG=1 diag`)
LIB_PATH = os.environ.get("GNNPE_LIB_PATH") or os.path.join(_HERE, "libgnnpe_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "gnnpe_hip.h")

_u32p = C.POINTER(C.c_uint32)
_u64p = C.POINTER(C.c_uint64)
_f64p = C.POINTER(C.c_double)
_vp = C.c_void_p

# name -> (restype, argtypes): one row per declaration in include/gnnpe_hip.h
SIGNATURES = {
    "gnnpe_abi_version": (C.c_int, []),
    "gnnpe_last_error": (C.c_char_p, []),
    "gnnpe_create": (_vp, [C.c_int]),
    "gnnpe_destroy": (None, [_vp]),
    "gnnpe_set_stream": (C.c_int, [_vp, _vp]),
    "gnnpe_sync": (C.c_int, [_vp]),
    "gnnpe_dev_alloc": (C.c_int, [_vp, C.c_uint64, C.POINTER(_vp)]),
    "gnnpe_dev_free": (C.c_int, [_vp, _vp]),
    "gnnpe_copy_to_host": (C.c_int, [_vp, _vp, _vp, C.c_uint64]),
    "gnnpe_device_count": (C.c_int, []),
    "gnnpe_get_stream": (C.c_int, [_vp, C.POINTER(_vp)]),
    "gnnpe_copy_device": (C.c_int, [_vp, _vp, _vp, C.c_uint64]),
    "gnnpe_gather_rows_device": (C.c_int, [_vp, C.c_uint64, C.c_uint32, _vp, C.c_uint64, _vp, _vp]),
    "gnnpe_write_device_file": (C.c_int, [_vp, _vp, C.c_uint64, C.c_char_p]),
    "gnnpe_load_csr": (C.c_int, [_vp, C.c_uint32, _u32p, _u32p, _u32p]),
    "gnnpe_load_rows": (C.c_int, [_vp, C.c_uint32, _u32p, C.c_uint32, _u32p, _u64p, _u32p, C.c_uint64]),
    "gnnpe_set_order": (C.c_int, [_vp, _u32p, _u32p, C.c_uint32]),
    "gnnpe_set_slab": (C.c_int, [_vp, C.c_uint32, C.c_uint32]),
    "gnnpe_set_label_table": (C.c_int, [_vp, C.c_uint32, C.c_uint32, _f64p]),
    "gnnpe_host_label_table": (C.c_int, [C.c_uint32, C.c_uint32, _f64p]),
    "gnnpe_host_load_graph": (C.c_int, [C.c_char_p, _u32p, _u32p, C.POINTER(_u32p), C.POINTER(_u32p), C.POINTER(_u32p),
                                        _u32p]),
    "gnnpe_host_load_multigraph": (C.c_int, [C.c_char_p, _u32p, _u32p, C.POINTER(_u32p), C.POINTER(_u32p), C.POINTER(_u32p),
                                             _u32p, C.POINTER(_u32p), C.POINTER(_u32p)]),
    "gnnpe_set_multigraph_rows": (C.c_int, [_vp, C.c_uint32, _u64p, _u32p]),
    "gnnpe_host_read_membership": (C.c_int, [C.c_char_p, C.c_uint32, C.c_uint32, _u32p, _u32p]),
    "gnnpe_host_free": (None, [_vp]),
    "gnnpe_host_csr_apply_edges": (C.c_int, [C.c_uint32, _u32p, _u32p, _u32p, C.c_uint64, _u32p, C.c_uint64, _u32p, _u32p, C.c_uint64,
                                             _u64p]),
    "gnnpe_csr_apply_edges": (C.c_int, [_vp, _u32p, C.c_uint64, _u32p, C.c_uint64, _u64p, _f64p]),
    "gnnpe_csr_download": (C.c_int, [_vp, _u32p, _u32p, C.c_uint64, _u64p]),
    "gnnpe_host_csr_entry_map": (C.c_int, [C.c_uint32, _u32p, _u32p, _u32p, _u32p, _u32p]),
    "gnnpe_csr_apply_edges_map": (C.c_int, [_vp, _u32p, C.c_uint64, _u32p, C.c_uint64, _u64p, _u64p, C.POINTER(_vp), _f64p]),
    "gnnpe_csr_carry_entries": (C.c_int, [_vp, C.c_uint32, C.c_uint32, _vp, _vp, _f64p]),
    "gnnpe_table_fold": (C.c_int, [_vp, _vp, _vp, C.c_uint64, _vp, _vp, C.c_uint64, _u64p, _f64p]),
    "gnnpe_host_csr_edges_below": (C.c_int, [C.c_uint32, _u32p, _u32p, _u64p, C.c_uint32, C.c_uint64, _u32p, C.c_uint64, _u64p, _u64p]),
    "gnnpe_csr_edges_below": (C.c_int, [_vp, _vp, C.c_uint32, C.c_uint64, _vp, C.c_uint64, _u64p, _u64p, _f64p]),
    "gnnpe_set_vertex_labels": (C.c_int, [_vp, _u32p, _u32p, C.c_uint64, _f64p]),
    "gnnpe_labels_download": (C.c_int, [_vp, _u32p]),
    "gnnpe_host_csr_apply_vertices": (C.c_int, [C.c_uint32, _u32p, _u32p, _u32p, _u32p, C.c_uint64, _u32p, C.c_uint64, _u32p, _u32p, C.c_uint64,
                                                _u32p, _u32p, _u32p, _u64p]),
    "gnnpe_csr_apply_vertices": (C.c_int, [_vp, _u32p, C.c_uint64, _u32p, C.c_uint64, _u32p, _u64p, _u64p, C.POINTER(_vp), C.POINTER(_vp),
                                           _f64p]),
    "gnnpe_csr_carry_vertices": (C.c_int, [_vp, C.c_uint32, C.c_uint32, _vp, _vp, _f64p]),
    "gnnpe_halo_need": (C.c_int, [_vp, C.c_uint32, _u32p, _vp, C.c_uint64, _u64p]),
    "gnnpe_rows_degree": (C.c_int, [_vp, C.c_uint64, _vp, _vp]),
    "gnnpe_rows_pack": (C.c_int, [_vp, C.c_uint64, _vp, _vp, C.c_uint64]),
    "gnnpe_rows_append": (C.c_int, [_vp, C.c_uint64, _vp, _vp, _vp, C.c_uint64, C.c_uint32]),
    "gnnpe_rows_drop_halo": (C.c_int, [_vp]),
    "gnnpe_rows_held": (C.c_int, [_vp, _u64p, _u64p, _u32p]),
    "gnnpe_vde": (C.c_int, [_vp, _f64p, _f64p, _f64p]),
    "gnnpe_vde_device_ptr": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(_vp)]),
    "gnnpe_vde_pack_slab": (C.c_int, [_vp, C.c_uint32, C.c_uint32, _vp]),
    "gnnpe_vde_unpack_slab": (C.c_int, [_vp, C.c_uint32, C.c_uint32, _vp]),
    "gnnpe_vde_unpack_all": (C.c_int, [_vp, C.c_uint32, _u32p, C.c_uint32, C.c_uint32, _vp]),
    "gnnpe_count_paths": (C.c_int, [_vp, C.c_uint32, _u64p, _u64p]),
    "gnnpe_fill_paths": (C.c_int, [_vp, C.c_uint64, C.c_uint64, _u32p, _f64p, _f64p]),
    "gnnpe_fill_paths_device": (C.c_int, [_vp, C.c_uint64, C.c_uint64, _vp, _vp, _vp]),
    "gnnpe_build_index_partition_aux_device": (C.c_int, [_vp, C.c_uint32, C.POINTER(_vp), _u64p, C.POINTER(C.c_int32), C.POINTER(_vp),
                                                         C.POINTER(_vp), C.POINTER(_vp), _u32p]),
    "gnnpe_output_pool_create": (C.c_int, [_vp, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p)]),
    "gnnpe_output_pool_acquire": (C.c_int, [_vp, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), _u64p]),
    "gnnpe_output_pool_report": (C.c_int, [_vp, C.c_uint32, C.POINTER(C.c_float), _u32p, _u32p, C.POINTER(C.c_int)]),
    "gnnpe_output_pool_destroy": (None, [_vp]),
    "gnnpe_count_paths_enqueue": (C.c_int, [_vp, C.c_uint32]),
    "gnnpe_count_total": (C.c_int, [_vp, _u64p]),
    "gnnpe_count_total_device": (C.c_int, [_vp, _vp]),
    "gnnpe_fill_paths_capped_device": (C.c_int, [_vp, C.c_uint64, _vp, _vp]),
    "gnnpe_path_partitions_device": (C.c_int, [_vp, C.c_uint64, C.c_uint64, _vp]),
    "gnnpe_text_paths": (C.c_int, [_vp, C.c_uint64, C.c_uint32, _vp, _vp, C.c_uint64, _u64p]),
    "gnnpe_text_ids": (C.c_int, [_vp, C.c_uint64, _vp, _vp, C.c_uint64, _u64p]),
    "gnnpe_select_partition": (C.c_int, [_vp, C.c_uint64, _vp, C.c_uint32, C.c_uint64, _vp, _u64p]),
    "gnnpe_rows_checksum_device": (C.c_int, [_vp, C.c_uint64, C.c_uint32, _vp, C.c_uint64, _u64p]),
    "gnnpe_host_query_plan": (C.c_int, [C.c_char_p, C.c_uint32, _u32p, _u32p, C.POINTER(_u32p), C.POINTER(_u32p),
                                        C.POINTER(_u32p), C.POINTER(_f64p)]),
    "gnnpe_host_load_path_sidecar": (C.c_int, [C.c_char_p, C.c_char_p, C.c_uint32, _u32p, _u32p, _u64p, _u32p, _u32p,
                                               C.POINTER(_u32p), C.POINTER(_u32p), C.POINTER(_u32p), C.POINTER(_f64p),
                                               C.POINTER(_f64p)]),
    "gnnpe_host_write_paths_header": (C.c_int, [_vp, C.c_uint32, C.c_uint64]),
    "gnnpe_host_load_partition_sidecar": (C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.c_uint32, _u32p, _u32p, _u64p, _u32p,
                                                    _u32p, C.POINTER(_u32p), C.POINTER(_u32p), C.POINTER(_u32p),
                                                    C.POINTER(_u32p), C.POINTER(_f64p), C.POINTER(_f64p)]),
    "gnnpe_aux_index_device": (C.c_int, [_vp, _vp, C.c_uint64, C.c_uint64, C.c_uint32, _vp, C.POINTER(_vp), C.POINTER(_vp),
                                         C.POINTER(_vp), _u32p, _u32p]),
    "gnnpe_build_aux_index": (C.c_int, [_vp, C.c_uint32, C.c_char_p]),
    "gnnpe_host_load_aux_index": (C.c_int, [C.c_char_p, _u32p, _u32p, _u32p, C.POINTER(_f64p), C.POINTER(_u32p),
                                            C.POINTER(_f64p)]),
    "gnnpe_pinned_alloc": (C.c_int, [C.c_uint64, C.POINTER(_vp)]),
    "gnnpe_pinned_free": (None, [_vp]),
    "gnnpe_set_degrees": (C.c_int, [_vp, _u32p]),
    "gnnpe_filter_candidates": (C.c_int, [_vp, C.c_uint32, _u32p, _u32p, _u32p, _f64p, C.c_uint32, C.c_double, _u32p,
                                          _f64p]),
    "gnnpe_host_query_plan_exact": (C.c_int, [C.c_char_p, C.c_uint32, C.c_uint32, _u32p, _u32p, C.POINTER(_u32p),
                                              C.POINTER(_u32p), C.POINTER(_u32p), C.POINTER(_f64p)]),
    "gnnpe_filter_candidates_exact": (C.c_int, [_vp, C.c_uint32, _u32p, _u32p, _u32p, _u32p, _f64p, C.c_uint32, C.c_double,
                                                _u32p, _f64p]),
    "gnnpe_filter_support_exact": (C.c_int, [_vp, C.c_uint32, _u32p, _u32p, _u32p, _u32p, _f64p, C.c_uint32, C.c_double, _vp,
                                             _f64p]),
    "gnnpe_filter_support_exact_delta": (C.c_int, [_vp, C.c_uint32, _u32p, _u32p, _u32p, _u32p, _f64p, C.c_uint32, C.c_double,
                                                   _u32p, C.c_uint64, C.c_int, _vp, _f64p]),
    "gnnpe_filter_support_exact_delta_device": (C.c_int, [_vp, C.c_uint32, _u32p, _u32p, _u32p, _u32p, _f64p, C.c_uint32, C.c_double,
                                                          _vp, _vp, C.c_uint64, C.c_int, _vp, _f64p]),
    "gnnpe_csr_closed_neighbourhood": (C.c_int, [_vp, _u32p, C.c_uint64, _vp, _vp, C.c_uint64, _u64p, _f64p]),
    "gnnpe_csr_carry_vertex_set": (C.c_int, [_vp, _vp, C.c_int, _vp, _vp, C.c_uint64, _u64p, _f64p]),
    "gnnpe_filter_support_bitmap": (C.c_int, [_vp, C.c_uint32, _vp, _u32p, _f64p]),
    "gnnpe_filter_support_bitmap_device": (C.c_int, [_vp, C.c_uint32, _vp, _vp, _f64p]),
    "gnnpe_build_index_device": (C.c_int, [_vp, C.c_uint64, C.c_uint32, _vp, C.POINTER(_vp), _u64p,
                                           C.POINTER(C.c_int32)]),
    "gnnpe_build_index": (C.c_int, [_vp, C.c_uint32, C.c_char_p]),
    "gnnpe_build_index_files": (C.c_int, [_vp, C.c_uint32, C.POINTER(C.c_char_p), C.POINTER(C.c_char_p)]),
    "gnnpe_build_index_partition_device": (C.c_int, [_vp, C.c_uint32, C.POINTER(_vp), _u64p, C.POINTER(C.c_int32)]),
    "gnnpe_build_box_index_device": (C.c_int, [_vp, C.c_uint64, C.c_uint32, _vp, C.POINTER(_vp), _u64p,
                                               C.POINTER(C.c_int32)]),
    "gnnpe_pge_groups": (C.c_int, [_vp, _f64p, _f64p]),
    "gnnpe_pge_device_ptr": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(_vp)]),
    "gnnpe_pge_build_index": (C.c_int, [_vp, C.c_uint64, _u32p, C.c_char_p]),
    "gnnpe_host_pge_query_groups": (C.c_int, [C.c_char_p, C.c_uint32, _u32p, C.POINTER(_u32p), C.POINTER(_u32p),
                                              C.POINTER(_f64p), C.POINTER(_f64p)]),
    "gnnpe_pge_set_groups": (C.c_int, [_vp, _f64p, _f64p]),
    "gnnpe_pge_filter_candidates": (C.c_int, [_vp, C.c_uint32, _u32p, _u32p, _f64p, _f64p, _u32p, _f64p]),
    "gnnpe_fill_kernel_name": (C.c_char_p, []),
    "gnnpe_set_fill_variant": (C.c_int, [_vp, C.c_int]),
    "gnnpe_set_emit_shape": (C.c_int, [_vp, C.c_int]),
    "gnnpe_index_file_bytes": (C.c_uint64, [C.c_uint64, C.c_uint32, C.c_int]),
    "gnnpe_emit_kernel_name": (C.c_char_p, [_vp]),
    "gnnpe_emit_calibrate_device": (C.c_int, [_vp, C.c_uint64, _vp, _vp, C.POINTER(C.c_float), C.POINTER(C.c_int)]),
}

ABI_VERSION = 20  # GNNPE_ABI_VERSION of include/gnnpe_hip.h
MATCH_DISTINCT, MATCH_INDUCED = 1, 2  # GNNPE_MATCH_* of include/gnnpe_online.h: the mode word of the gnnpe_*_mode functions
_lib = None


class GnnpeError(RuntimeError):
    pass


# include/gnnpe_online.h (libgnnpe_online.so): the refinement -- out of SURVEY section 8's scope, a library of its own since round 6
ONLINE_LIB_PATH = os.path.join(_HERE, "libgnnpe_online.so")
ONLINE_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "gnnpe_online.h")
ONLINE_SIGNATURES = {
    # the standing exact query
    "gnnpe_standing_open": (C.c_int, [_vp, C.c_char_p, C.c_uint32, C.c_double, C.c_uint32, C.c_uint64, C.POINTER(_vp), _u64p, _f64p]),
    "gnnpe_standing_open_sets": (C.c_int, [_vp, C.c_char_p, C.c_uint32, C.c_uint64, _u32p, C.POINTER(_vp), _u64p, _f64p]),
    "gnnpe_standing_set_bitmap": (C.c_int, [_vp, _u32p]),
    "gnnpe_standing_apply_edges": (C.c_int, [_vp, _u32p, C.c_uint64, _u32p, C.c_uint64, _f64p]),
    "gnnpe_standing_set_labels": (C.c_int, [_vp, _u32p, _u32p, C.c_uint64, _f64p]),
    "gnnpe_standing_apply_vertices": (C.c_int, [_vp, _u32p, C.c_uint64, _u32p, C.c_uint64, _u32p, _f64p]),
    "gnnpe_standing_result": (C.c_int, [_vp, _u64p]),
    "gnnpe_standing_rows": (C.c_int, [_vp, C.c_int, _u32p, C.c_uint64, _u64p]),
    "gnnpe_standing_set_sizes": (C.c_int, [_vp, _u64p]),
    "gnnpe_standing_set_members": (C.c_int, [_vp, C.c_uint32, _u32p, C.c_uint64, _u64p]),
    "gnnpe_standing_bitmap": (C.c_int, [_vp, _u32p]),
    "gnnpe_standing_table": (C.c_int, [_vp, C.POINTER(_vp)]),
    "gnnpe_standing_keep_counts": (C.c_int, [_vp, C.c_uint32, C.c_uint64, _f64p]),
    "gnnpe_standing_counts": (C.c_int, [_vp, C.c_uint32, _u64p, C.POINTER(_vp), _u64p, _u64p]),
    "gnnpe_standing_count_changes": (C.c_int, [_vp, C.c_uint32, _u64p, C.POINTER(C.c_int64), C.c_uint64, _u64p]),
    "gnnpe_standing_peel": (C.c_int, [_vp, C.c_uint64, C.c_uint32, _u32p, _u32p, C.c_uint64, _u64p, _f64p]),
    "gnnpe_standing_truss_levels": (C.c_int, [_vp, C.c_int, _u32p, _u64p, C.c_uint64, _u64p, _f64p]),
    "gnnpe_host_truss_levels": (C.c_int, [C.c_uint32, _u32p, _u32p, _u32p, C.c_char_p, _u32p, C.c_uint32, _u32p, _u64p, C.c_uint64, _u64p]),
    "gnnpe_standing_refresh": (C.c_int, [_vp, _u64p, _f64p]),
    "gnnpe_standing_close": (C.c_int, [_vp]),
    "gnnpe_host_refine": (C.c_int, [C.c_uint32, _u32p, _u32p, _u32p, C.c_char_p, _u32p, C.c_uint64, _u64p]),
    "gnnpe_refine": (C.c_int, [_vp, C.c_char_p, _u32p, C.c_uint64, _u64p, _f64p]),
    "gnnpe_host_refine_sets": (C.c_int, [C.c_uint32, _u32p, _u32p, _u32p, C.c_char_p, _u32p, C.c_uint64, _u64p]),
    "gnnpe_refine_sets": (C.c_int, [_vp, C.c_char_p, _u32p, C.c_uint64, _u64p, _u32p, C.c_uint64, _f64p]),
    "gnnpe_refine_pages_open": (C.c_int, [_vp, C.c_char_p, _u32p, C.c_uint64, C.c_uint64, C.POINTER(_vp)]),
    "gnnpe_refine_pages_next": (C.c_int, [_vp, _u32p, _u64p, C.POINTER(C.c_int), _f64p]),
    "gnnpe_refine_pages_device_ptr": (C.c_int, [_vp, C.POINTER(_vp), _u32p]),
    "gnnpe_refine_pages_info": (C.c_int, [_vp, _u64p]),
    "gnnpe_refine_pages_close": (None, [_vp]),
    "gnnpe_host_query_symmetry": (C.c_int, [C.c_char_p, _u64p, _u32p, C.c_uint32, _u32p]),
    "gnnpe_host_refine_sets_distinct": (C.c_int, [C.c_uint32, _u32p, _u32p, _u32p, C.c_char_p, _u32p, C.c_uint64, _u64p]),
    "gnnpe_refine_sets_distinct": (C.c_int, [_vp, C.c_char_p, _u32p, C.c_uint64, _u64p, _u32p, C.c_uint64, _f64p]),
    "gnnpe_refine_pages_open_distinct": (C.c_int, [_vp, C.c_char_p, _u32p, C.c_uint64, C.c_uint64, C.POINTER(_vp)]),
    "gnnpe_host_refine_sets_mode": (C.c_int, [C.c_uint32, _u32p, _u32p, _u32p, C.c_char_p, _u32p, C.c_uint64, C.c_uint32, _u64p]),
    "gnnpe_refine_sets_mode": (C.c_int, [_vp, C.c_char_p, _u32p, C.c_uint64, C.c_uint32, _u64p, _u32p, C.c_uint64, _f64p]),
    "gnnpe_refine_pages_open_mode": (C.c_int, [_vp, C.c_char_p, _u32p, C.c_uint64, C.c_uint64, C.c_uint32, C.POINTER(_vp)]),
    "gnnpe_refine_pages_open_delta": (C.c_int, [_vp, C.c_char_p, _u32p, _u32p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, C.POINTER(_vp)]),
    "gnnpe_refine_pages_open_delta_nonedges": (C.c_int, [_vp, C.c_char_p, _u32p, _u32p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, C.POINTER(_vp)]),
    "gnnpe_refine_pages_open_delta_vertices": (C.c_int, [_vp, C.c_char_p, _u32p, _u32p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, C.POINTER(_vp)]),
    "gnnpe_host_refine_sets_vertex_counts": (C.c_int, [C.c_uint32, _u32p, _u32p, _u32p, C.c_char_p, _u32p, C.c_uint64, C.c_uint32,
                                                       _u64p, C.POINTER(C.c_int), _u64p]),
    "gnnpe_refine_sets_vertex_counts": (C.c_int, [_vp, C.c_char_p, _u32p, C.c_uint64, C.c_uint32, _u64p, C.POINTER(C.c_int), _u64p,
                                                  C.POINTER(_vp), _f64p]),
    "gnnpe_host_query_edges": (C.c_int, [C.c_char_p, _u32p, C.c_uint32, _u32p]),
    "gnnpe_host_refine_sets_edge_counts": (C.c_int, [C.c_uint32, _u32p, _u32p, _u32p, C.c_char_p, _u32p, C.c_uint64, C.c_uint32,
                                                     _u64p, C.POINTER(C.c_int), _u64p]),
    "gnnpe_refine_sets_edge_counts": (C.c_int, [_vp, C.c_char_p, _u32p, C.c_uint64, C.c_uint32, _u64p, C.POINTER(C.c_int), _u64p,
                                                C.POINTER(_vp), _f64p]),
    "gnnpe_host_refine_sets_delta": (C.c_int, [C.c_uint32, _u32p, _u32p, _u32p, C.c_char_p, _u32p, _u32p, C.c_uint64, C.c_uint64,
                                               C.c_uint32, _u64p]),
    "gnnpe_refine_sets_delta": (C.c_int, [_vp, C.c_char_p, _u32p, _u32p, C.c_uint64, C.c_uint64, C.c_uint32, _u64p, _u32p, C.c_uint64,
                                          _f64p]),
    "gnnpe_host_refine_sets_delta_vertex_counts": (C.c_int, [C.c_uint32, _u32p, _u32p, _u32p, C.c_char_p, _u32p, _u32p, C.c_uint64,
                                                             C.c_uint64, C.c_uint32, _u64p, C.POINTER(C.c_int), _u64p]),
    "gnnpe_host_refine_sets_delta_edge_counts": (C.c_int, [C.c_uint32, _u32p, _u32p, _u32p, C.c_char_p, _u32p, _u32p, C.c_uint64,
                                                           C.c_uint64, C.c_uint32, _u64p, C.POINTER(C.c_int), _u64p]),
    "gnnpe_refine_sets_delta_vertex_counts": (C.c_int, [_vp, C.c_char_p, _u32p, _u32p, C.c_uint64, C.c_uint64, C.c_uint32, _u64p,
                                                        C.POINTER(C.c_int), _u64p, C.POINTER(_vp), _vp, C.c_int, _f64p]),
    "gnnpe_refine_sets_delta_edge_counts": (C.c_int, [_vp, C.c_char_p, _u32p, _u32p, C.c_uint64, C.c_uint64, C.c_uint32, _u64p,
                                                      C.POINTER(C.c_int), _u64p, C.POINTER(_vp), _vp, C.c_int, _f64p]),
    "gnnpe_host_query_nonedges": (C.c_int, [C.c_char_p, _u32p, C.c_uint32, _u32p]),
    "gnnpe_host_refine_sets_delta_nonedges": (C.c_int, [C.c_uint32, _u32p, _u32p, _u32p, C.c_char_p, _u32p, _u32p, C.c_uint64,
                                                        C.c_uint64, C.c_uint32, _u64p]),
    "gnnpe_refine_sets_delta_nonedges": (C.c_int, [_vp, C.c_char_p, _u32p, _u32p, C.c_uint64, C.c_uint64, C.c_uint32, _u64p, _u32p,
                                                   C.c_uint64, _f64p]),
    "gnnpe_host_refine_sets_delta_nonedges_vertex_counts": (C.c_int, [C.c_uint32, _u32p, _u32p, _u32p, C.c_char_p, _u32p, _u32p,
                                                                      C.c_uint64, C.c_uint64, C.c_uint32, _u64p, C.POINTER(C.c_int),
                                                                      _u64p]),
    "gnnpe_host_refine_sets_delta_nonedges_edge_counts": (C.c_int, [C.c_uint32, _u32p, _u32p, _u32p, C.c_char_p, _u32p, _u32p,
                                                                    C.c_uint64, C.c_uint64, C.c_uint32, _u64p, C.POINTER(C.c_int), _u64p]),
    "gnnpe_refine_sets_delta_nonedges_vertex_counts": (C.c_int, [_vp, C.c_char_p, _u32p, _u32p, C.c_uint64, C.c_uint64, C.c_uint32,
                                                                 _u64p, C.POINTER(C.c_int), _u64p, C.POINTER(_vp), _vp, C.c_int, _f64p]),
    "gnnpe_refine_sets_delta_nonedges_edge_counts": (C.c_int, [_vp, C.c_char_p, _u32p, _u32p, C.c_uint64, C.c_uint64, C.c_uint32, _u64p,
                                                               C.POINTER(C.c_int), _u64p, C.POINTER(_vp), _vp, C.c_int, _f64p]),
    "gnnpe_host_refine_sets_delta_vertices": (C.c_int, [C.c_uint32, _u32p, _u32p, _u32p, C.c_char_p, _u32p, _u32p, C.c_uint64,
                                                        C.c_uint64, C.c_uint32, _u64p]),
    "gnnpe_refine_sets_delta_vertices": (C.c_int, [_vp, C.c_char_p, _u32p, _u32p, C.c_uint64, C.c_uint64, C.c_uint32, _u64p, _u32p,
                                                   C.c_uint64, _f64p]),
    "gnnpe_host_refine_sets_delta_vertices_vertex_counts": (C.c_int, [C.c_uint32, _u32p, _u32p, _u32p, C.c_char_p, _u32p, _u32p,
                                                                      C.c_uint64, C.c_uint64, C.c_uint32, _u64p, C.POINTER(C.c_int),
                                                                      _u64p]),
    "gnnpe_host_refine_sets_delta_vertices_edge_counts": (C.c_int, [C.c_uint32, _u32p, _u32p, _u32p, C.c_char_p, _u32p, _u32p,
                                                                    C.c_uint64, C.c_uint64, C.c_uint32, _u64p, C.POINTER(C.c_int), _u64p]),
    "gnnpe_refine_sets_delta_vertices_vertex_counts": (C.c_int, [_vp, C.c_char_p, _u32p, _u32p, C.c_uint64, C.c_uint64, C.c_uint32,
                                                                 _u64p, C.POINTER(C.c_int), _u64p, C.POINTER(_vp), _vp, C.c_int, _f64p]),
    "gnnpe_refine_sets_delta_vertices_edge_counts": (C.c_int, [_vp, C.c_char_p, _u32p, _u32p, C.c_uint64, C.c_uint64, C.c_uint32, _u64p,
                                                               C.POINTER(C.c_int), _u64p, C.POINTER(_vp), _vp, C.c_int, _f64p]),
}
_online = None


def load_online():
    """dlopen libgnnpe_online.so (it links against libgnnpe_hip.so, which load() brings in first).  Raises if absent."""
    global _online
    if _online is not None:
        return _online
    load()
    if not os.path.exists(ONLINE_LIB_PATH):
        raise GnnpeError(f"{ONLINE_LIB_PATH} is missing: build it with `make -C gnn-pe_amd`")
    lib = C.CDLL(ONLINE_LIB_PATH)
    for name, (res, args) in ONLINE_SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _online = lib
    return lib


def build(force=False):
    """Compile libgnnpe_hip.so for gfx950 with hipcc (cross-compiles without a GPU)."""
    srcs = [os.path.join(_HERE, "csrc", f) for f in os.listdir(os.path.join(_HERE, "csrc"))] + [HEADER_PATH]
    stale = (not os.path.exists(LIB_PATH)) or any(os.path.getmtime(s) > os.path.getmtime(LIB_PATH) for s in srcs)
    if force or stale:
        subprocess.check_call(["make", "-C", _HERE, "libgnnpe_hip.so", "libgnnpe_online.so"])
    return LIB_PATH


def load():
    """dlopen libgnnpe_hip.so and bind every symbol the header declares.  Raises if absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise GnnpeError(f"{LIB_PATH} is missing: build it with `make -C gnn-pe_amd` "
                         "(there is no CPU fallback for the HIP engine)")
    try:
        # torch bundles its own libamdhip64 (same SONAME as /opt/rocm's): whichever is loaded first
        # serves the whole process, and torch cannot initialise on the other one.  Load torch's first.
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the library does not export the symbol
        fn.restype = res
        fn.argtypes = args
    if lib.gnnpe_abi_version() != ABI_VERSION:
        raise GnnpeError(f"ABI version {lib.gnnpe_abi_version()} != {ABI_VERSION}")
    _lib = lib
    return lib


def _np(a, dtype):
    return None if a is None else np.ascontiguousarray(a, dtype)


def _ptr(a, t):
    return None if a is None else a.ctypes.data_as(t)


def _dev(t):
    """Raw device pointer of a torch tensor / int / None."""
    if t is None:
        return None
    if isinstance(t, int):
        return C.c_void_p(t)
    return C.c_void_p(t.data_ptr())


def host_label_table(n_labels, e):
    """R3: gen_vde_x (custom.h:492-511) for labels 0..n_labels-1 -- host arithmetic inside the library."""
    out = np.zeros((n_labels, e))
    rc = load().gnnpe_host_label_table(n_labels, e, _ptr(out, _f64p))
    if rc:
        raise GnnpeError(load().gnnpe_last_error().decode())
    return out


def simple_rows(offsets, nbrs):
    """The rows the reference's DFS + hash set amount to (custom.h:68-77): every ascending list without its repeats.
    offsets [n + 1], nbrs: a CSR as graph.cpp:211-233 leaves a file with duplicate `e` lines.  Returns (offsets, nbrs) uint32."""
    offsets, nbrs = _np(offsets, np.uint32), _np(nbrs, np.uint32)
    n = len(offsets) - 1
    row = np.repeat(np.arange(n, dtype=np.uint32), np.diff(offsets.astype(np.int64)))
    keep = np.ones(len(nbrs), bool)
    if len(nbrs):
        keep[1:] = (nbrs[1:] != nbrs[:-1]) | (row[1:] != row[:-1])
    so = np.zeros(n + 1, np.uint32)
    so[1:] = np.cumsum(np.bincount(row[keep], minlength=n))
    return so, np.ascontiguousarray(nbrs[keep])


def host_load_graph(path, strict=True):
    """R0 through the library's own loader (host/graph_loader.cpp).  Returns a dict like synth graphs.  strict=False: a file with
    duplicate `e` lines is loaded as the reference loads it (offsets / nbrs keep the repeats) and the dict also holds
    simple_offsets / simple_nbrs, the rows the enumeration runs on (None for a simple graph).  Self-loops are refused either way
    (the reference's loader leaves a slot uninitialised for them: graph.cpp:211-218)."""
    lib = load()
    n, m = C.c_uint32(), C.c_uint32()
    po, pn, pl = _u32p(), _u32p(), _u32p()
    meta = (C.c_uint32 * 3)()
    if not strict:
        pso, psn = _u32p(), _u32p()
        rc = lib.gnnpe_host_load_multigraph(path.encode(), C.byref(n), C.byref(m), C.byref(po), C.byref(pn), C.byref(pl), meta,
                                            C.byref(pso), C.byref(psn))
    else:
        rc = lib.gnnpe_host_load_graph(path.encode(), C.byref(n), C.byref(m), C.byref(po), C.byref(pn), C.byref(pl), meta)
    if rc == -1:
        raise FileNotFoundError(lib.gnnpe_last_error().decode())
    if rc:
        raise GnnpeError(lib.gnnpe_last_error().decode())
    offs = np.ctypeslib.as_array(po, shape=(n.value + 1,)).copy()
    nbrs = np.ctypeslib.as_array(pn, shape=(max(2 * m.value, 1),)).copy()[: 2 * m.value]
    labels = np.ctypeslib.as_array(pl, shape=(max(n.value, 1),)).copy()[: n.value]
    extra = {}
    if not strict:
        if pso:
            so = np.ctypeslib.as_array(pso, shape=(n.value + 1,)).copy()
            extra = dict(simple_offsets=so, simple_nbrs=np.ctypeslib.as_array(psn, shape=(max(int(so[-1]), 1),)).copy()[: int(so[-1])])
            lib.gnnpe_host_free(pso)
            lib.gnnpe_host_free(psn)
        else:
            extra = dict(simple_offsets=None, simple_nbrs=None)
    for p in (po, pn, pl):
        lib.gnnpe_host_free(p)
    return dict(n=n.value, m=m.value, offsets=offs, nbrs=nbrs, labels=labels, labels_count=meta[0], max_degree=meta[1],
                max_label_frequency=meta[2], **extra)


def host_query_plan(path, e):
    """Query side of the online filter (main.cpp:136-151) through the library's host planner.
    Returns dict(n_vertices, vids, labels, degrees (n_paths x 3), pde (n_paths x 3e))."""
    lib = load()
    nv, npth = C.c_uint32(), C.c_uint32()
    pv, pl, pd = _u32p(), _u32p(), _u32p()
    pp = _f64p()
    rc = lib.gnnpe_host_query_plan(path.encode(), int(e), C.byref(nv), C.byref(npth), C.byref(pv), C.byref(pl), C.byref(pd),
                                   C.byref(pp))
    if rc == -1:
        raise FileNotFoundError(lib.gnnpe_last_error().decode())
    if rc:
        raise GnnpeError(lib.gnnpe_last_error().decode())
    k = npth.value
    out = dict(n_vertices=nv.value)
    for name, ptr in (("vids", pv), ("labels", pl), ("degrees", pd)):
        out[name] = np.ctypeslib.as_array(ptr, shape=(max(k * 3, 1),)).copy()[: k * 3].reshape(k, 3)
        lib.gnnpe_host_free(ptr)
    out["pde"] = np.ctypeslib.as_array(pp, shape=(max(k * 3 * e, 1),)).copy()[: k * 3 * e].reshape(k, 3 * e)
    lib.gnnpe_host_free(pp)
    return out


def host_query_plan_exact(path, e, l):
    """Exact-mode plan (include/gnnpe_hip.h, gnnpe_host_query_plan_exact) at l = 2 or 3.  Returns dict(n_vertices, l, e,
    main=(vids, labels, degrees: n x (l+1); pde: n x (l+1)e), tri=(the same at width 3), single=(width 1: the vde of the
    vertex in pde)), each part a dict of those four arrays."""
    lib = load()
    nv = C.c_uint32()
    counts = (C.c_uint32 * 3)()
    pv, pl, pd = _u32p(), _u32p(), _u32p()
    pp = _f64p()
    rc = lib.gnnpe_host_query_plan_exact(path.encode(), int(e), int(l), C.byref(nv), counts, C.byref(pv), C.byref(pl),
                                         C.byref(pd), C.byref(pp))
    if rc == -1:
        raise FileNotFoundError(lib.gnnpe_last_error().decode())
    if rc:
        raise GnnpeError(lib.gnnpe_last_error().decode())
    widths = (int(l) + 1, 3, 1)
    k = sum(c * w for c, w in zip(counts, widths))
    flat = {}
    for name, ptr in (("vids", pv), ("labels", pl), ("degrees", pd)):
        flat[name] = np.ctypeslib.as_array(ptr, shape=(max(k, 1),)).copy()[:k]
        lib.gnnpe_host_free(ptr)
    flat["pde"] = np.ctypeslib.as_array(pp, shape=(max(k * e, 1),)).copy()[: k * e]
    lib.gnnpe_host_free(pp)
    out = dict(n_vertices=nv.value, l=int(l), e=int(e))
    o = 0
    for part, c, w in zip(("main", "tri", "single"), counts, widths):
        out[part] = dict(vids=flat["vids"][o:o + c * w].reshape(c, w), labels=flat["labels"][o:o + c * w].reshape(c, w),
                         degrees=flat["degrees"][o:o + c * w].reshape(c, w),
                         pde=flat["pde"][o * e:(o + c * w) * e].reshape(c, w * e))
        o += c * w
    return out


def host_pge_query_groups(path, e):
    """GNN-PGE query side (GNN-PGE/src/main.cpp:253-329) through the library's host code.  Returns dict(n_vertices,
    labels, degrees (n), pg, plg (n x 4e)).  A query vertex without an edge raises GnnpeError."""
    lib = load()
    nv = C.c_uint32()
    pl, pd = _u32p(), _u32p()
    pg, plg = _f64p(), _f64p()
    rc = lib.gnnpe_host_pge_query_groups(path.encode(), int(e), C.byref(nv), C.byref(pl), C.byref(pd), C.byref(pg), C.byref(plg))
    if rc == -1:
        raise FileNotFoundError(lib.gnnpe_last_error().decode())
    if rc:
        raise GnnpeError(f"[{rc}] " + lib.gnnpe_last_error().decode())
    n, w = nv.value, 4 * int(e)
    out = dict(n_vertices=n)
    for name, ptr in (("labels", pl), ("degrees", pd)):
        out[name] = np.ctypeslib.as_array(ptr, shape=(max(n, 1),)).copy()[:n]
        lib.gnnpe_host_free(ptr)
    for name, ptr in (("pg", pg), ("plg", plg)):
        out[name] = np.ctypeslib.as_array(ptr, shape=(max(n * w, 1),)).copy()[: n * w].reshape(n, w)
        lib.gnnpe_host_free(ptr)
    return out


def host_refine(g, query_path, bitmap, limit=0xFFFFFFFF):
    """Refinement half of the online step on the host (custom.h:634-932): answer count from the filter's bitmap."""
    lib = load()
    out = C.c_uint64()
    o, nb, lb = _np(g["offsets"], np.uint32), _np(g["nbrs"], np.uint32), _np(g["labels"], np.uint32)
    bm = _np(bitmap, np.uint32)
    rc = load_online().gnnpe_host_refine(len(o) - 1, _ptr(o, _u32p), _ptr(nb, _u32p), _ptr(lb, _u32p), query_path.encode(),
                               _ptr(bm, _u32p), int(limit), C.byref(out))
    if rc:
        raise GnnpeError(lib.gnnpe_last_error().decode())
    return out.value


def match_mode(distinct=False, induced=False):
    """the mode word of the gnnpe_*_mode functions"""
    return (MATCH_DISTINCT if distinct else 0) | (MATCH_INDUCED if induced else 0)


def _bitmap_rows(bm, n):
    """query vertices of a bitmap: its rows, or for a flat one its words over ceil(n / 32)"""
    return bm.shape[0] if bm.ndim == 2 else bm.size // max((n + 31) // 32, 1)


def _delta_pairs(edges):
    """F of the delta calls as a contiguous (n_delta, 2) uint32 array; ids that do not fit 32 bits are refused here"""
    e = np.asarray(edges, np.int64).reshape(-1, 2)
    if e.size and (e.min() < 0 or e.max() > 0xFFFFFFFF):
        raise GnnpeError("delta edges: vertex ids are uint32")
    return np.ascontiguousarray(e, np.uint32)


def _table_ptr(table):
    """device address of a caller's table: a torch tensor or anything with data_ptr(), or the address itself"""
    if table is None:
        return None
    return C.c_void_p(int(table.data_ptr()) if hasattr(table, "data_ptr") else int(table))


def _vertex_ids(vertices):
    """S of the vertex-anchored calls as a contiguous uint32 array; ids that do not fit 32 bits are refused here"""
    v = np.asarray(vertices, np.int64).reshape(-1)
    if v.size and (v.min() < 0 or v.max() > 0xFFFFFFFF):
        raise GnnpeError("vertices: vertex ids are uint32")
    return np.ascontiguousarray(v, np.uint32)


def _host_sets(entry, g, query_path, bitmap, limit, mode=None, edges=None, shape=None, vertices=None):
    """One call of a host entry of the set-restricted refinement (include/gnnpe_online.h): g, the bitmap, F where `edges` is
    given (S where `vertices` is), the mode word unless `mode` is None (the two entries without one), and a zeroed table where
    `shape` is given.
    Returns answers, or with a table (answers, complete, counts); a refusal raises GnnpeError with the library's text."""
    lib = load()
    out, done = C.c_uint64(), C.c_int()
    o, nb, lb = _np(g["offsets"], np.uint32), _np(g["nbrs"], np.uint32), _np(g["labels"], np.uint32)
    bm = _np(bitmap, np.uint32)
    args = [len(o) - 1, _ptr(o, _u32p), _ptr(nb, _u32p), _ptr(lb, _u32p), query_path.encode(), _ptr(bm, _u32p)]
    if edges is not None:
        e = _delta_pairs(edges)
        args += [_ptr(e, _u32p) if len(e) else None, len(e)]
    if vertices is not None:
        s = _vertex_ids(vertices)
        args += [_ptr(s, _u32p) if len(s) else None, len(s)]
    args += [int(limit)] + ([] if mode is None else [mode]) + [C.byref(out)]
    if shape is not None:
        counts = np.zeros(shape, np.uint64)
        args += [C.byref(done), _ptr(counts, _u64p)]
    if getattr(load_online(), entry)(*args):
        raise GnnpeError(lib.gnnpe_last_error().decode())
    return out.value if shape is None else (out.value, bool(done.value), counts)


def host_refine_sets(g, query_path, bitmap, limit=0xFFFFFFFF, distinct=False, induced=False):
    """Set-restricted refinement on the host (include/gnnpe_online.h, R(C, limit)): the embeddings whose every image lies in its
    query vertex's set, counted up to `limit`.  distinct=True: D(C, limit), one embedding per distinct subgraph.  induced=True:
    I(C, limit) (with distinct ID): only the maps that send non-adjacent query vertices to non-adjacent data vertices."""
    if induced:
        return _host_sets("gnnpe_host_refine_sets_mode", g, query_path, bitmap, limit, match_mode(distinct, induced))
    # (the entries of ABI 9 and ABI 11, which take no mode word)
    return _host_sets("gnnpe_host_refine_sets_distinct" if distinct else "gnnpe_host_refine_sets", g, query_path, bitmap, limit)


def host_refine_sets_vertex_counts(g, query_path, bitmap, limit=2 ** 64 - 1, distinct=False, induced=False):
    """Per-vertex match counts on the host (include/gnnpe_online.h, V_m(C)): (answers, complete, counts) with counts[u, v] = the
    matches of the mode that send query vertex u to data vertex v, an (nq, n) uint64 array; nq is taken from the bitmap's rows.
    `limit` is a guard: answers = min(matches, limit), complete = matches < limit, and counts is exact only where complete."""
    bm, n = _np(bitmap, np.uint32), len(g["offsets"]) - 1
    return _host_sets("gnnpe_host_refine_sets_vertex_counts", g, query_path, bm, limit, match_mode(distinct, induced),
                      shape=(_bitmap_rows(bm, n), n))


def host_query_edges(query_path):
    """gnnpe_host_query_edges: the query edges as the edge-count tables number them, an (nqe, 2) uint32 array of (a_k, b_k) with
    a_k < b_k, lexicographically ascending."""
    lib, online = load(), load_online()
    k = C.c_uint32()
    online.gnnpe_host_query_edges(query_path.encode(), None, 0, C.byref(k))  # (a file that does not load fails again below)
    edges = np.zeros((max(k.value, 1), 2), np.uint32)
    if online.gnnpe_host_query_edges(query_path.encode(), _ptr(edges, _u32p), k.value, C.byref(k)):
        raise GnnpeError(lib.gnnpe_last_error().decode())
    return edges[:k.value].copy()


def _edge_table_shape(g, query_path):
    return len(host_query_edges(query_path)), int(np.asarray(g["offsets"])[-1])


def host_refine_sets_edge_counts(g, query_path, bitmap, limit=2 ** 64 - 1, distinct=False, induced=False):
    """Per-edge match counts on the host (include/gnnpe_online.h, E_m(C)): (answers, complete, counts) with counts[k, j] = the
    matches of the mode that send query edge k = host_query_edges(query_path)[k] = (a, b) onto adjacency entry j of g: a to the
    vertex whose row holds j, b to g["nbrs"][j]; an (nqe, len(g["nbrs"])) uint64 array.  `limit` is a guard: answers =
    min(matches, limit), complete = matches < limit, and counts is exact only where complete."""
    return _host_sets("gnnpe_host_refine_sets_edge_counts", g, query_path, bitmap, limit, match_mode(distinct, induced),
                      shape=_edge_table_shape(g, query_path))


def host_refine_sets_delta(g, query_path, bitmap, edges, limit=2 ** 64 - 1, distinct=False, induced=False):
    """The matches through a set of data edges on the host (include/gnnpe_online.h, Delta_m(C, F, limit)): the number of matches
    of the mode that put at least one query edge on one of `edges` (pairs (x, y), either orientation, repeats tolerated), each
    match once, up to `limit`.  A pair that is no edge of g, a loop or an id outside g raises GnnpeError."""
    return _host_sets("gnnpe_host_refine_sets_delta", g, query_path, bitmap, limit, match_mode(distinct, induced), edges)


def host_refine_sets_delta_vertices(g, query_path, bitmap, vertices, limit=2 ** 64 - 1, distinct=False, induced=False):
    """The matches through a set of data vertices on the host (include/gnnpe_online.h, DeltaV_m(C, S, limit)): the number of
    matches of the mode with at least one image among `vertices` (ids, repeats tolerated), each match once, up to `limit`.  An id
    outside g raises GnnpeError."""
    return _host_sets("gnnpe_host_refine_sets_delta_vertices", g, query_path, bitmap, limit, match_mode(distinct, induced),
                      vertices=vertices)


def host_refine_sets_delta_vertices_vertex_counts(g, query_path, bitmap, vertices, limit=2 ** 64 - 1, distinct=False, induced=False):
    """The per-vertex table of the matches through a set of data vertices on the host (include/gnnpe_online.h, VV_m(C, S)):
    (answers, complete, counts) as host_refine_sets_vertex_counts, over the matches host_refine_sets_delta_vertices counts only;
    answers = min(DeltaV, limit), complete = DeltaV < limit.  `vertices` as for host_refine_sets_delta_vertices."""
    bm, n = _np(bitmap, np.uint32), len(g["offsets"]) - 1
    return _host_sets("gnnpe_host_refine_sets_delta_vertices_vertex_counts", g, query_path, bm, limit, match_mode(distinct, induced),
                      shape=(_bitmap_rows(bm, n), n), vertices=vertices)


def host_refine_sets_delta_vertices_edge_counts(g, query_path, bitmap, vertices, limit=2 ** 64 - 1, distinct=False, induced=False):
    """The per-edge table of the matches through a set of data vertices on the host (include/gnnpe_online.h, EV_m(C, S)): (answers,
    complete, counts) as host_refine_sets_edge_counts, over the matches host_refine_sets_delta_vertices counts only."""
    return _host_sets("gnnpe_host_refine_sets_delta_vertices_edge_counts", g, query_path, bitmap, limit, match_mode(distinct, induced),
                      shape=_edge_table_shape(g, query_path), vertices=vertices)


def host_refine_sets_delta_vertex_counts(g, query_path, bitmap, edges, limit=2 ** 64 - 1, distinct=False, induced=False):
    """The per-vertex table of the matches through a set of data edges on the host (include/gnnpe_online.h, ABI 17): (answers,
    complete, counts) as host_refine_sets_vertex_counts, over the matches host_refine_sets_delta counts only; answers =
    min(Delta, limit), complete = Delta < limit.  `edges` as for host_refine_sets_delta."""
    bm, n = _np(bitmap, np.uint32), len(g["offsets"]) - 1
    return _host_sets("gnnpe_host_refine_sets_delta_vertex_counts", g, query_path, bm, limit, match_mode(distinct, induced), edges,
                      (_bitmap_rows(bm, n), n))


def host_refine_sets_delta_edge_counts(g, query_path, bitmap, edges, limit=2 ** 64 - 1, distinct=False, induced=False):
    """The per-edge table of the matches through a set of data edges on the host (include/gnnpe_online.h, ABI 17): (answers,
    complete, counts) as host_refine_sets_edge_counts, over the matches host_refine_sets_delta counts only."""
    return _host_sets("gnnpe_host_refine_sets_delta_edge_counts", g, query_path, bitmap, limit, match_mode(distinct, induced), edges,
                      _edge_table_shape(g, query_path))


def host_query_nonedges(query_path):
    """gnnpe_host_query_nonedges: the non-adjacent pairs of the query as ABI 18 numbers them, an (nqn, 2) uint32 array of (a_k, b_k)
    with a_k < b_k, lexicographically ascending."""
    lib, online = load(), load_online()
    k = C.c_uint32()
    online.gnnpe_host_query_nonedges(query_path.encode(), None, 0, C.byref(k))  # (a file that does not load fails again below)
    pairs = np.zeros((max(k.value, 1), 2), np.uint32)
    if online.gnnpe_host_query_nonedges(query_path.encode(), _ptr(pairs, _u32p), k.value, C.byref(k)):
        raise GnnpeError(lib.gnnpe_last_error().decode())
    return pairs[:k.value].copy()


def host_refine_sets_delta_nonedges(g, query_path, bitmap, pairs, limit=2 ** 64 - 1, distinct=False):
    """The induced matches on a set of non-edges on the host (include/gnnpe_online.h, N_m(C, F, limit), ABI 18): the number of induced
    matches (with distinct=True of the INDUCED | DISTINCT mode) that put at least one non-adjacent query pair on one of `pairs`
    ((x, y), either orientation, repeats tolerated), each match once, up to `limit`.  A pair that is an edge of g, a loop or an id
    outside g raises GnnpeError."""
    return _host_sets("gnnpe_host_refine_sets_delta_nonedges", g, query_path, bitmap, limit, match_mode(distinct, True), pairs)


def host_refine_sets_delta_nonedges_vertex_counts(g, query_path, bitmap, pairs, limit=2 ** 64 - 1, distinct=False):
    """The per-vertex table of the induced matches on a set of non-edges on the host (include/gnnpe_online.h, VN_m(C, F), ABI 19):
    (answers, complete, counts) as host_refine_sets_vertex_counts, over the matches host_refine_sets_delta_nonedges counts only;
    answers = min(N, limit), complete = N < limit.  `pairs` as for host_refine_sets_delta_nonedges."""
    bm, n = _np(bitmap, np.uint32), len(g["offsets"]) - 1
    return _host_sets("gnnpe_host_refine_sets_delta_nonedges_vertex_counts", g, query_path, bm, limit, match_mode(distinct, True), pairs,
                      (_bitmap_rows(bm, n), n))


def host_refine_sets_delta_nonedges_edge_counts(g, query_path, bitmap, pairs, limit=2 ** 64 - 1, distinct=False):
    """The per-edge table of the induced matches on a set of non-edges on the host (include/gnnpe_online.h, EN_m(C, F), ABI 19):
    (answers, complete, counts) as host_refine_sets_edge_counts -- the rows are the query EDGES of host_query_edges -- over the
    matches host_refine_sets_delta_nonedges counts only."""
    return _host_sets("gnnpe_host_refine_sets_delta_nonedges_edge_counts", g, query_path, bitmap, limit, match_mode(distinct, True), pairs,
                      _edge_table_shape(g, query_path))


def host_apply_edges(g, insert=None, delete=None):
    """gnnpe_host_csr_apply_edges: the graph dict of G' = (E(g) minus delete) plus insert, a compact CSR with g's labels.  The
    lists hold pairs (x, y), either orientation, repeats tolerated; a loop, an id outside g, an insertion that is an edge, a
    deletion that is none or an edge in both lists raises GnnpeError."""
    lib = load()
    o, nb = _np(g["offsets"], np.uint32), _np(g["nbrs"], np.uint32)
    ins, dele = _delta_pairs([] if insert is None else insert), _delta_pairs([] if delete is None else delete)
    n = len(o) - 1
    cap = len(nb) + 2 * len(ins)
    out_o, out_nb, after = np.zeros(n + 1, np.uint32), np.zeros(cap, np.uint32), C.c_uint64()
    rc = lib.gnnpe_host_csr_apply_edges(n, _ptr(o, _u32p), _ptr(nb, _u32p), _ptr(ins, _u32p) if len(ins) else None, len(ins),
                                        _ptr(dele, _u32p) if len(dele) else None, len(dele), _ptr(out_o, _u32p),
                                        _ptr(out_nb, _u32p), cap, C.byref(after))
    if rc:
        raise GnnpeError(f"[{rc}] " + lib.gnnpe_last_error().decode())
    out = dict(g)
    out["offsets"], out["nbrs"] = out_o, out_nb[:after.value].copy()
    return out


NO_ENTRY = 0xFFFFFFFF  # GNNPE_NO_ENTRY of include/gnnpe_hip.h


def host_entry_map(g_old, g_new):
    """gnnpe_host_csr_entry_map: for every adjacency entry (x -> y) of g_new the index of the entry (x -> y) in g_old, NO_ENTRY
    where g_old does not have it, as a uint32 array; both are compact simple CSRs on the same vertices."""
    lib = load()
    o0, n0 = _np(g_old["offsets"], np.uint32), _np(g_old["nbrs"], np.uint32)
    o1, n1 = _np(g_new["offsets"], np.uint32), _np(g_new["nbrs"], np.uint32)
    if len(o0) != len(o1):
        raise GnnpeError("host_entry_map: the two graphs have different vertex counts")
    out = np.zeros(len(n1), np.uint32)
    rc = lib.gnnpe_host_csr_entry_map(len(o0) - 1, _ptr(o0, _u32p), _ptr(n0, _u32p), _ptr(o1, _u32p), _ptr(n1, _u32p), _ptr(out, _u32p))
    if rc:
        raise GnnpeError(f"[{rc}] " + lib.gnnpe_last_error().decode())
    return out


def host_edges_below(g, table, threshold, cap=None):
    """gnnpe_host_csr_edges_below: the undirected edges of g whose support in `table` (n_rows x entries uint64: the sum over the
    rows of the cells of the edge's two entries, mod 2^64) is below `threshold`, as ascending (x, y) pairs with x < y.  Returns
    (the first min(cap, n_selected) pairs as an (k, 2) uint32 array, n_selected, min_kept); cap=None: room for every edge."""
    lib = load()
    off, nb = _np(g["offsets"], np.uint32), _np(g["nbrs"], np.uint32)
    tab = np.ascontiguousarray(table, np.uint64)
    if tab.ndim != 2 or tab.shape[1] != len(nb):
        raise GnnpeError(f"host_edges_below: the table is {tab.shape}, the graph has {len(nb)} entries")
    cap = len(nb) // 2 if cap is None else int(cap)
    pairs, n_sel, low = np.zeros((max(cap, 1), 2), np.uint32), C.c_uint64(), C.c_uint64()
    rc = lib.gnnpe_host_csr_edges_below(len(off) - 1, _ptr(off, _u32p), _ptr(nb, _u32p), _ptr(tab, _u64p), tab.shape[0],
                                        int(threshold), _ptr(pairs, _u32p) if cap else None, cap, C.byref(n_sel), C.byref(low))
    if rc:
        raise GnnpeError(f"[{rc}] " + lib.gnnpe_last_error().decode())
    return pairs[:min(cap, n_sel.value)].copy(), int(n_sel.value), int(low.value)


def host_truss_levels(g, query_path, bitmap, distinct=False):
    """gnnpe_host_truss_levels: the truss level of every edge of g for the query (include/gnnpe_online.h, "PEELING THE GRAPH BY EDGE
    SUPPORT"), by peeling with a full recount every round: (edges (m, 2) uint32 in removal order, levels uint64, out) with out =
    [edges, distinct levels, largest level, rounds]."""
    lib, online = load(), load_online()
    off, nb, lab = _np(g["offsets"], np.uint32), _np(g["nbrs"], np.uint32), _np(g["labels"], np.uint32)
    bm = _np(bitmap, np.uint32)
    m = len(nb) // 2
    edges, levels, out = np.zeros((max(m, 1), 2), np.uint32), np.zeros(max(m, 1), np.uint64), (C.c_uint64 * 4)()
    rc = online.gnnpe_host_truss_levels(len(off) - 1, _ptr(off, _u32p), _ptr(nb, _u32p), _ptr(lab, _u32p), query_path.encode(), _ptr(bm, _u32p),
                                        match_mode(distinct, False), _ptr(edges, _u32p), _ptr(levels, _u64p), m, out)
    if rc:
        raise GnnpeError(f"[{rc}] " + lib.gnnpe_last_error().decode())
    return edges[:out[0]].copy(), levels[:out[0]].copy(), [int(x) for x in out]


NO_VERTEX = 0xFFFFFFFF  # GNNPE_NO_VERTEX of include/gnnpe_hip.h


def host_apply_vertices(g, remove=None, add_labels=None):
    """gnnpe_host_csr_apply_vertices: (g2, vertex_map).  g2 is the graph dict of g without the vertices of `remove` (ids of g,
    repeats tolerated) and their edges, the survivors in their order under new ids, and with one vertex per label of add_labels
    appended, each with an empty row.  vertex_map[v'] is the id in g of vertex v' of g2, NO_VERTEX for an added one.  An id
    outside g or a batch that leaves no vertex raises GnnpeError."""
    lib = load()
    o, nb, lab = _np(g["offsets"], np.uint32), _np(g["nbrs"], np.uint32), _np(g["labels"], np.uint32)
    rem, add = _vertex_ids([] if remove is None else remove), _vertex_ids([] if add_labels is None else add_labels)
    n = len(o) - 1
    room = n + len(add)  # n' is at most this
    out_o, out_nb, out_lab, vmap = np.zeros(room + 1, np.uint32), np.zeros(len(nb), np.uint32), np.zeros(room, np.uint32), np.zeros(room, np.uint32)
    n2, after = C.c_uint32(), C.c_uint64()
    rc = lib.gnnpe_host_csr_apply_vertices(n, _ptr(o, _u32p), _ptr(nb, _u32p), _ptr(lab, _u32p), _ptr(rem, _u32p) if len(rem) else None, len(rem),
                                           _ptr(add, _u32p) if len(add) else None, len(add), _ptr(out_o, _u32p), _ptr(out_nb, _u32p),
                                           len(out_nb), _ptr(out_lab, _u32p), _ptr(vmap, _u32p), C.byref(n2), C.byref(after))
    if rc:
        raise GnnpeError(f"[{rc}] " + lib.gnnpe_last_error().decode())
    out = dict(g)
    out["n"] = int(n2.value)
    out["offsets"], out["nbrs"] = out_o[:n2.value + 1].copy(), out_nb[:after.value].copy()
    out["labels"] = out_lab[:n2.value].copy()
    return out, vmap[:n2.value].copy()


def host_query_symmetry(query_path, pairs_cap=None):
    """gnnpe_host_query_symmetry: (|Aut(Q)| saturated at 2^64 - 1, pairs ndarray [k, 2]); a pair (a, b) asks for f(a) < f(b), and of
    the |Aut(Q)| embeddings of one subgraph exactly one satisfies every pair.  pairs_cap (default: whatever is needed) is the room
    offered to the library; too little raises with the needed number in the message."""
    lib, online = load(), load_online()
    aut, k = C.c_uint64(), C.c_uint32()
    if pairs_cap is None:
        online.gnnpe_host_query_symmetry(query_path.encode(), C.byref(aut), None, 0, C.byref(k))
        pairs_cap = k.value
    pairs = np.zeros((max(int(pairs_cap), 1), 2), np.uint32)
    rc = online.gnnpe_host_query_symmetry(query_path.encode(), C.byref(aut), _ptr(pairs, _u32p), int(pairs_cap), C.byref(k))
    if rc:
        raise GnnpeError(lib.gnnpe_last_error().decode())
    return aut.value, pairs[:k.value].copy()


def host_load_path_sidecar(paths_bin, vde_bin, labels, degrees):
    """gen_pde's per-path arrays (custom.h:546-572) from the binary sidecars of `gnnpe_main --sidecars`."""
    lib = load()
    lab, deg = _np(labels, np.uint32), _np(degrees, np.uint32)
    P, L, e = C.c_uint64(), C.c_uint32(), C.c_uint32()
    pv, pl, pd = _u32p(), _u32p(), _u32p()
    pp, px = _f64p(), _f64p()
    rc = lib.gnnpe_host_load_path_sidecar(paths_bin.encode(), vde_bin.encode(), len(lab), _ptr(lab, _u32p), _ptr(deg, _u32p),
                                          C.byref(P), C.byref(L), C.byref(e), C.byref(pv), C.byref(pl), C.byref(pd), C.byref(pp),
                                          C.byref(px))
    if rc:
        raise GnnpeError(lib.gnnpe_last_error().decode())
    n, Lv, D = P.value, L.value, L.value * e.value
    out = {}
    for name, ptr, w in (("vids", pv, Lv), ("labels", pl, Lv), ("degrees", pd, Lv), ("pde", pp, D), ("pde_label", px, D)):
        out[name] = np.ctypeslib.as_array(ptr, shape=(max(n * w, 1),)).copy()[: n * w].reshape(n, w)
        lib.gnnpe_host_free(ptr)
    return out


def host_load_partition_sidecar(paths_bin, vde_bin, partition_paths_txt, labels, degrees):
    """the partition's copy of the paths (Partition::Partition, custom.h:205-216) from the sidecars and the
    partition's partition_paths.txt: gen_pde's arrays for its rows only, plus the global path ids."""
    lib = load()
    lab, deg = _np(labels, np.uint32), _np(degrees, np.uint32)
    P, L, e = C.c_uint64(), C.c_uint32(), C.c_uint32()
    pi, pv, pl, pd = _u32p(), _u32p(), _u32p(), _u32p()
    pp, px = _f64p(), _f64p()
    rc = lib.gnnpe_host_load_partition_sidecar(paths_bin.encode(), vde_bin.encode(), partition_paths_txt.encode(), len(lab),
                                               _ptr(lab, _u32p), _ptr(deg, _u32p), C.byref(P), C.byref(L), C.byref(e),
                                               C.byref(pi), C.byref(pv), C.byref(pl), C.byref(pd), C.byref(pp), C.byref(px))
    if rc:
        raise GnnpeError(lib.gnnpe_last_error().decode())
    n, Lv, D = P.value, L.value, L.value * e.value
    out = {}
    for name, ptr, w in (("path_ids", pi, 1), ("vids", pv, Lv), ("labels", pl, Lv), ("degrees", pd, Lv), ("pde", pp, D),
                         ("pde_label", px, D)):
        out[name] = np.ctypeslib.as_array(ptr, shape=(max(n * w, 1),)).copy()[: n * w].reshape(n, w)
        lib.gnnpe_host_free(ptr)
    out["path_ids"] = out["path_ids"].reshape(-1)
    return out


def host_load_aux_index(path):
    """aux_index.bin -> what Partition::build_auxiliary_index (custom.h:268-364) computes, by node block id."""
    lib = load()
    N, L, D = C.c_uint32(), C.c_uint32(), C.c_uint32()
    pk, pd, pm = _f64p(), _u32p(), _f64p()
    rc = lib.gnnpe_host_load_aux_index(path.encode(), C.byref(N), C.byref(L), C.byref(D), C.byref(pk), C.byref(pd), C.byref(pm))
    if rc:
        raise GnnpeError(lib.gnnpe_last_error().decode())
    n = N.value
    out = dict(L=L.value, D=D.value)
    for name, ptr, w in (("key", pk, 1), ("degrees", pd, L.value), ("label_mbr", pm, 2 * D.value)):
        out[name] = np.ctypeslib.as_array(ptr, shape=(max(n * w, 1),)).copy()[: n * w].reshape(n, w)
        lib.gnnpe_host_free(ptr)
    out["key"] = out["key"].reshape(-1)
    return out


def host_read_membership(path, n, p):
    """R1 (main.cpp:77-85) through the library's reader."""
    lib = load()
    sn = np.zeros(n, np.uint32)
    mem = np.zeros(n, np.uint32)
    rc = lib.gnnpe_host_read_membership(path.encode(), n, p, _ptr(sn, _u32p), _ptr(mem, _u32p))
    if rc:
        raise GnnpeError(lib.gnnpe_last_error().decode())
    return sn, mem


class _DevArray:
    """A typed view of raw device memory for torch (`torch.as_tensor(view, device=...)` shares it, no copy)."""

    def __init__(self, ptr, shape, typestr, owner=None):
        self.owner = owner  # keeps the pool (and through it the engine) alive for as long as a tensor shares the memory
        self.shape = tuple(int(x) for x in shape)
        self.__cuda_array_interface__ = dict(shape=tuple(int(x) for x in shape), typestr=typestr, data=(int(ptr), False),
                                             version=2, strides=None)


class OutputPool:
    """gnnpe_output_pool_*: the emit kernel's output buffers (ids: rows_cap x L uint32, pde: rows_cap x D doubles).  One
    allocation by default; with `candidates` > 1 the fastest of that many independent allocations, each timed with the emit
    kernel (or, without a count on the engine, a streaming write), the others freed before the constructor returns.  With an
    l = 2 count on the engine the pool also times both emit shapes into the buffer it keeps (gnnpe_emit_calibrate_device).
    `ids` / `pde` are raw device pointers (ints); ids_tensor() / pde_tensor() are torch views of the same memory: close() refuses
    while one of them is alive (Engine.close() does not ask -- drop the views before closing the engine).  Create the pool
    AFTER eng.count_paths() so that the probe is the emit kernel itself."""

    NO_CALIBRATION = 0x80000000  # GNNPE_POOL_NO_CALIBRATION

    def __init__(self, eng, rows_cap, L, D, candidates=1, calibrate=True):
        self.eng, self.lib = eng, eng.lib
        self.rows_cap, self.L, self.D = int(max(rows_cap, 1)), int(L), int(D)
        h = C.c_void_p()
        eng._ck(self.lib.gnnpe_output_pool_create(eng.ctx, self.rows_cap, self.L, self.D, int(candidates) | (0 if calibrate else self.NO_CALIBRATION), C.byref(h)))
        self.h = h
        self._views = []  # weak references to the arrays handed to torch
        eng._pools.append(self)
        self._refresh()

    def _refresh(self):
        a, b, cap = C.c_void_p(), C.c_void_p(), C.c_uint64()
        self.eng._ck(self.lib.gnnpe_output_pool_acquire(self.h, C.byref(a), C.byref(b), C.byref(cap)))
        self.ids, self.pde = int(a.value or 0), int(b.value or 0)

    def report(self):
        ms = (C.c_float * 64)()
        n, kept, kern = C.c_uint32(), C.c_uint32(), C.c_int()
        self.eng._ck(self.lib.gnnpe_output_pool_report(self.h, 64, ms, C.byref(n), C.byref(kept), C.byref(kern)))
        return dict(candidates_ms=[round(float(ms[i]), 4) for i in range(n.value)], kept=int(kept.value),
                    probe="emit kernel" if kern.value else "streaming write")

    def ids_tensor(self, device):
        import torch
        return torch.as_tensor(self._view(self.ids, (self.rows_cap, self.L), "<i4"), device=device)

    def pde_tensor(self, device):
        import torch
        return torch.as_tensor(self._view(self.pde, (self.rows_cap, self.D), "<f8"), device=device) if self.D else None

    def _view(self, ptr, shape, typestr):
        import weakref
        a = _DevArray(ptr, shape, typestr, owner=self)
        self._views.append(weakref.ref(a))
        return a

    def close(self, force=False):
        """Frees the pool's memory.  A pool never outlives its engine: Engine.close() closes its pools first (force)."""
        if not force and any(r() is not None for r in self._views):
            raise GnnpeError("OutputPool.close(): a tensor from ids_tensor() / pde_tensor() still shares the pool's memory; drop it first")
        if self.h and self.eng.ctx:
            self.lib.gnnpe_output_pool_destroy(self.h)
            if self in self.eng._pools:
                self.eng._pools.remove(self)
        self.h = None

    def __del__(self):
        try:
            self.close(force=True)
        except Exception:
            pass


class MatchCursor:
    """gnnpe_refine_pages_*: a cursor over the embeddings of a query inside its candidate sets.  next() delivers the next page of
    at most page_rows embeddings as (rows, done); across the pages every embedding comes out exactly once, up to `limit`.  With
    device=False rows is a fresh np.uint32 array of n_rows x n_query_vertices; with device=True it is a zero-copy view of the
    cursor's device page (`torch.as_tensor(rows, device=...)` shares it: int32 words holding the uint32 ids, like
    OutputPool.ids_tensor), valid until the next next() or close().  distinct=True: one embedding per distinct subgraph
    (gnnpe_refine_pages_open_distinct); induced=True: induced matches only (gnnpe_refine_pages_open_mode).  Loading another graph into the engine invalidates the
    cursor: next() raises.  Engine.close() closes the engine's open cursors."""

    INFO_FIELDS = ("pages", "rows", "suspended_waves", "items_left", "slots")

    def __init__(self, eng, query_path, bitmap, page_rows, limit=2 ** 64 - 1, device=False, distinct=False, induced=False, anchor=None):
        self.eng, self.lib, self.h = eng, load_online(), None
        bm = _np(bitmap, np.uint32)
        self.page_rows, self.device = int(page_rows), bool(device)
        self.done = False
        h = C.c_void_p()
        if anchor is not None:
            # a delta cursor: anchor = (suffix of gnnpe_refine_pages_open_delta, F as pairs or S as ids)
            sfx, ids = anchor
            eng._ck(getattr(self.lib, "gnnpe_refine_pages_open_delta" + sfx)(eng.ctx, query_path.encode(), _ptr(bm, _u32p),
                                                                            _ptr(ids, _u32p) if len(ids) else None, len(ids), int(limit),
                                                                            self.page_rows, match_mode(distinct, induced), C.byref(h)))
        elif induced:
            eng._ck(self.lib.gnnpe_refine_pages_open_mode(eng.ctx, query_path.encode(), _ptr(bm, _u32p), int(limit), self.page_rows,
                                                          match_mode(distinct, induced), C.byref(h)))
        else:
            open_fn = self.lib.gnnpe_refine_pages_open_distinct if distinct else self.lib.gnnpe_refine_pages_open
            eng._ck(open_fn(eng.ctx, query_path.encode(), _ptr(bm, _u32p), int(limit), self.page_rows, C.byref(h)))
        self.h = h
        ptr, nq = C.c_void_p(), C.c_uint32()
        eng._ck(self.lib.gnnpe_refine_pages_device_ptr(self.h, C.byref(ptr), C.byref(nq)))
        self.nq = int(nq.value)
        self._host_rows = min(self.page_rows, int(limit))  # rows a page can hold
        eng._cursors.append(self)

    def next(self):
        """(rows, done): the next page; after done, an empty page and done again"""
        if not self.h:
            raise GnnpeError("MatchCursor.next(): the cursor is closed")
        n, done, ms = C.c_uint64(), C.c_int(), C.c_double()
        rows = None if self.device or self.done else np.empty((self._host_rows, self.nq), np.uint32)
        self.eng._ck(self.lib.gnnpe_refine_pages_next(self.h, _ptr(rows, _u32p), C.byref(n), C.byref(done), C.byref(ms)))
        self.done, self.device_ms = bool(done.value), ms.value
        k = int(n.value)
        if not self.device:
            return (np.zeros((0, self.nq), np.uint32) if rows is None else rows[:k].copy() if k < len(rows) else rows), self.done
        ptr = C.c_void_p()
        self.eng._ck(self.lib.gnnpe_refine_pages_device_ptr(self.h, C.byref(ptr), None))
        return _DevArray(int(ptr.value or 0), (k, self.nq), "<i4", owner=self), self.done

    def info(self):
        out = (C.c_uint64 * 5)()
        self.eng._ck(self.lib.gnnpe_refine_pages_info(self.h, out))
        return dict(zip(self.INFO_FIELDS, (int(x) for x in out)))

    def close(self):
        if self.h and self.eng.ctx:
            self.lib.gnnpe_refine_pages_close(self.h)
        self.h = None
        if self in self.eng._cursors:
            self.eng._cursors.remove(self)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class StandingQuery:
    """A standing exact query (gnnpe_standing_* of include/gnnpe_online.h): the parsed query, the support table S of the exact
    filter, the candidate bitmap C and the exact match count stay on the device, and Engine.standing_apply_edges moves the graph
    and every open handle forward by an edge batch.  Made by Engine.standing_open.  count / created / destroyed: the count on the
    current graph and what the last batch created and destroyed.  Every call but refresh() and close() raises GnnpeError once the
    graph, the labels or the label table changed behind the handle."""

    def __init__(self, eng, query_path, l, eps, mode, rows_cap, bitmap):
        self.eng, self.handle = eng, _vp()
        self.online = load_online()
        count, ms = C.c_uint64(), C.c_double()
        if bitmap is None:
            rc = self.online.gnnpe_standing_open(eng.ctx, query_path.encode(), int(l), float(eps), mode, int(rows_cap),
                                                 C.byref(self.handle), C.byref(count), C.byref(ms))
        else:
            bm = _np(bitmap, np.uint32)
            rc = self.online.gnnpe_standing_open_sets(eng.ctx, query_path.encode(), mode, int(rows_cap), _ptr(bm, _u32p),
                                                      C.byref(self.handle), C.byref(count), C.byref(ms))
        eng._ck(rc)
        self.open_ms = ms.value
        self.changes_cap = 0  # of keep_counts
        self.nq = len(self.set_sizes())
        eng._standing.append(self)

    def result(self):
        """(count, created, destroyed, rows_created, rows_destroyed, graph generation)"""
        out = (C.c_uint64 * 6)()
        self.eng._ck(self.online.gnnpe_standing_result(self.handle, out))
        return tuple(int(x) for x in out)

    count = property(lambda self: self.result()[0])
    created = property(lambda self: self.result()[1])
    destroyed = property(lambda self: self.result()[2])

    def rows(self, which, cap=None):
        """the kept rows of the last batch: which = 0 (or "created") / 1 (or "destroyed"); (rows, nq) uint32, column = query vertex"""
        which = {"created": 0, "destroyed": 1}.get(which, which)
        held = self.result()[3 + int(which)] if cap is None else int(cap)
        out, n = np.zeros((max(held, 1), self.nq), np.uint32), C.c_uint64()
        self.eng._ck(self.online.gnnpe_standing_rows(self.handle, int(which), _ptr(out, _u32p), held, C.byref(n)))
        return out[:min(held, n.value)]

    def set_sizes(self):
        """|C(u)| of every query vertex, from k_sets_sizes"""
        out = (C.c_uint64 * 32)(*([2 ** 64 - 1] * 32))  # the library writes one value per query vertex, each below 2^32
        self.eng._ck(self.online.gnnpe_standing_set_sizes(self.handle, out))
        return np.array([x for x in out if x != 2 ** 64 - 1], np.uint64)

    def set_members(self, u, cap=None, out=None):
        """the ascending ids of C(u), from k_sets_members: (ids, size); with cap the first cap ids and the true size.  `out`: a
        uint32 array to write the ids into (its words beyond cap are left alone)."""
        cap = self.eng.n if cap is None else int(cap)
        buf = np.zeros(max(cap, 1), np.uint32) if out is None else out
        n = C.c_uint64()
        self.eng._ck(self.online.gnnpe_standing_set_members(self.handle, int(u), _ptr(buf, _u32p), cap, C.byref(n)))
        return buf[:min(cap, n.value)], int(n.value)

    def bitmap(self):
        """C as the host bitmap every refinement call takes: (nq, ceil(n / 32)) uint32"""
        bm = np.zeros((self.nq, (self.eng.n + 31) // 32), np.uint32)
        self.eng._ck(self.online.gnnpe_standing_bitmap(self.handle, _ptr(bm, _u32p)))
        return bm

    def set_bitmap(self, bitmap):
        """a new bitmap for a handle opened with one; the count is taken again"""
        bm = _np(bitmap, np.uint32)
        self.eng._ck(self.online.gnnpe_standing_set_bitmap(self.handle, _ptr(bm, _u32p)))

    def table_ptr(self):
        """device address of S (nq x n uint64), 0 for a handle opened with a bitmap"""
        p = _vp()
        self.eng._ck(self.online.gnnpe_standing_table(self.handle, C.byref(p)))
        return p.value or 0

    def table(self):
        """S on the host, (nq, n) uint64; None for a handle opened with a bitmap"""
        p = self.table_ptr()
        if not p:
            return None
        return self.eng.copy_to_host(p, self.nq * self.eng.n * 8).view(np.uint64).reshape(self.nq, self.eng.n)

    VERTEX_COUNTS, EDGE_COUNTS = 1, 2

    @staticmethod
    def _which(which):
        return {"vertex": 1, "edge": 2, "V": 1, "E": 2}.get(which, which)

    def keep_counts(self, vertex=True, edge=False, changes_cap=0, timing=False):
        """gnnpe_standing_keep_counts: from now on the handle keeps V (nq x n) and / or E (query edges x entries) exact across
        standing_apply_edges, and per batch the list of the cells that changed (the first changes_cap of them are held).  May be
        called again to add the other table or to change changes_cap.  Returns the device ms with timing."""
        ms = C.c_double()
        self.eng._ck(self.online.gnnpe_standing_keep_counts(self.handle, (1 if vertex else 0) | (2 if edge else 0), int(changes_cap),
                                                            C.byref(ms) if timing else None))
        self.changes_cap = int(changes_cap)
        return ms.value if timing else None

    def counts_ptr(self, which):
        """(device address of the kept table, rows, columns); which: 1 / "vertex" or 2 / "edge".  Valid until the next batch,
        refresh or close; 0 for a table without cells."""
        p, rows, cols = _vp(), C.c_uint64(), C.c_uint64()
        self.eng._ck(self.online.gnnpe_standing_counts(self.handle, self._which(which), None, C.byref(p), C.byref(rows), C.byref(cols)))
        return p.value or 0, rows.value, cols.value

    def counts(self, which):
        """the kept table on the host: (nq, n) or (query edges, entries) uint64"""
        _, rows, cols = self.counts_ptr(which)
        out = np.zeros((rows, cols), np.uint64)
        buf = out if out.size else np.zeros(1, np.uint64)
        self.eng._ck(self.online.gnnpe_standing_counts(self.handle, self._which(which), _ptr(buf, _u64p), None, None, None))
        return out

    def count_changes(self, which, cap=None):
        """the cells of the kept table the last batch changed: (cells uint64 ascending, deltas int64), the first min(cap,
        changes_cap, n_changes(which)) pairs.  A V cell is u * n + v, an E cell k * entries + j on the current graph."""
        which = self._which(which)
        cap = self.n_changes(which) if cap is None else int(cap)
        cells, deltas, n = np.zeros(max(cap, 1), np.uint64), np.zeros(max(cap, 1), np.int64), C.c_uint64()
        self.eng._ck(self.online.gnnpe_standing_count_changes(self.handle, which, _ptr(cells, _u64p), deltas.ctypes.data_as(C.POINTER(C.c_int64)),
                                                              cap, C.byref(n)))
        held = min(cap, self.changes_cap, n.value)
        return cells[:held], deltas[:held]

    def n_changes(self, which):
        """how many cells of the kept table the last batch changed, whatever changes_cap holds of them"""
        n = C.c_uint64()
        self.eng._ck(self.online.gnnpe_standing_count_changes(self.handle, self._which(which), None, None, 0, C.byref(n)))
        return int(n.value)

    def peel(self, min_support, max_rounds=0, timing=False):
        """gnnpe_standing_peel: rounds of "select the edges whose support in the kept E is below min_support on the device, delete
        them as one standing_apply_edges batch" until nothing is selected (max_rounds=0) or max_rounds rounds have deleted
        something.  Needs keep_counts(edge=True).  Returns (removed (k, 2) uint32 in removal order, their rounds uint32 counted
        from 1, out) with out = [rounds, edges removed, undirected edges left, converged]; the device ms appended with timing."""
        cap = self.eng.rows_held()[1] // 2
        removed, rounds = np.zeros((max(cap, 1), 2), np.uint32), np.zeros(max(cap, 1), np.uint32)
        out, ms = (C.c_uint64 * 4)(), C.c_double()
        rc = self.online.gnnpe_standing_peel(self.handle, int(min_support), int(max_rounds), _ptr(removed, _u32p), _ptr(rounds, _u32p), cap, out,
                                             C.byref(ms) if timing else None)
        self._graph_moved(out[0] != 0)  # (a peel that failed in a later round has moved the graph too)
        self.eng._ck(rc)
        res = (removed[:out[1]].copy(), rounds[:out[1]].copy(), [int(x) for x in out])
        return res + (ms.value,) if timing else res

    def _graph_moved(self, moved):
        """the engine's own bookkeeping after a call that applied batches inside the library, as standing_apply_edges keeps it"""
        eng = self.eng
        eng._map_call += 1
        if moved:
            eng._rows_gen += 1
            eng.slab = (0, eng.n)
            eng.entries = eng.rows_held()[1]

    def truss_levels(self, restore=True, timing=False):
        """gnnpe_standing_truss_levels: the truss level of every edge of the resident graph by peeling it level by level; with
        restore the removed edges are inserted again at the end, without it the context is left with the empty graph.  Returns
        (edges (m, 2) uint32 in removal order, levels uint64, out) with out = [edges, distinct levels, largest level, rounds]; the
        device ms appended with timing."""
        cap = self.eng.rows_held()[1] // 2
        edges, levels = np.zeros((max(cap, 1), 2), np.uint32), np.zeros(max(cap, 1), np.uint64)
        out, ms = (C.c_uint64 * 4)(), C.c_double()
        rc = self.online.gnnpe_standing_truss_levels(self.handle, 1 if restore else 0, _ptr(edges, _u32p), _ptr(levels, _u64p), cap, out,
                                                     C.byref(ms) if timing else None)
        self._graph_moved(out[0] != 0)
        self.eng._ck(rc)
        res = (edges[:out[0]].copy(), levels[:out[0]].copy(), [int(x) for x in out])
        return res + (ms.value,) if timing else res

    def refresh(self, timing=False):
        """S, C and the count again from the graph as it is now: the state of a fresh open"""
        count, ms = C.c_uint64(), C.c_double()
        self.eng._ck(self.online.gnnpe_standing_refresh(self.handle, C.byref(count), C.byref(ms) if timing else None))
        return (count.value, ms.value) if timing else count.value

    def close(self):
        if self.handle:
            if self.eng.ctx:
                self.online.gnnpe_standing_close(self.handle)
            self.handle = _vp()
            if self in self.eng._standing:
                self.eng._standing.remove(self)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Engine:
    """One context = one GPU.  Method names follow the reference functions they replace."""

    def __init__(self, device=0, stream=None):
        self.lib = load()
        self.ctx = self.lib.gnnpe_create(int(device))
        if not self.ctx:
            raise GnnpeError("gnnpe_create: " + self.lib.gnnpe_last_error().decode())
        self.device_index = int(device)
        self.n = 0
        self.e = 0
        self.entries = 0  # adjacency entries of the CSR given to load_csr: the width of the edge-count tables
        self._rows_gen = self._ecounts_call = 0  # what an edge-count device view is valid for
        # ... and a view of a delta table, or of a table over non-edges
        self._delta_counts_call = {"vertex": 0, "edge": 0, "nonedges_vertex": 0, "nonedges_edge": 0, "vertices_vertex": 0,
                                   "vertices_edge": 0}
        self._map_call = 0  # ... and a view of the entry map: every apply_edges / apply_edges_map ends the one before
        self.slab = (0, 0)
        self.total = None
        self._pools = []
        self._cursors = []  # open match cursors: closed before the context goes
        self._standing = []  # open standing queries: closed before the context goes
        self.stream_handle = None  # None = the context's own stream
        if stream is not None:
            self.set_stream(stream)

    def close(self):
        if self.ctx:
            for cur in list(getattr(self, "_cursors", [])):
                cur.close()
            for sq in list(getattr(self, "_standing", [])):
                sq.close()
            for p in list(getattr(self, "_pools", [])):
                p.close(force=True)
            self.lib.gnnpe_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc):
        if rc != 0:
            raise GnnpeError(f"[{rc}] " + self.lib.gnnpe_last_error().decode())

    def set_stream(self, stream):
        """stream: raw hipStream_t as int (torch.cuda.current_stream().cuda_stream), or None."""
        self._ck(self.lib.gnnpe_set_stream(self.ctx, C.c_void_p(stream) if stream else None))
        self.stream_handle = int(stream) if stream else None

    def sync(self):
        self._ck(self.lib.gnnpe_sync(self.ctx))

    # R0: Static_Graph::loadGraphFromFile output (graph.cpp:163-242)
    def load_csr(self, offsets, nbrs, labels):
        offsets, nbrs, labels = _np(offsets, np.uint32), _np(nbrs, np.uint32), _np(labels, np.uint32)
        n = len(offsets) - 1
        assert len(labels) == n and len(nbrs) == offsets[-1]
        self._rows_gen += 1
        self._ck(self.lib.gnnpe_load_csr(self.ctx, n, _ptr(offsets, _u32p), _ptr(nbrs, _u32p), _ptr(labels, _u32p)))
        self.n = n
        self.entries = int(offsets[-1])
        self.slab = (0, n)

    def load_multigraph(self, offsets, nbrs, labels):
        """R0 for a CSR with repeated entries, as the reference's loader leaves a file with duplicate `e` lines: the simple rows
        for the enumeration (custom.h:68-77), the stored rows for gen_vde and the degree columns (include/gnnpe_hip.h)."""
        so, sn = simple_rows(offsets, nbrs)
        self.load_csr(so, sn, labels)
        if len(sn) != len(nbrs):
            self.set_multigraph_rows(_np(offsets, np.uint32).astype(np.uint64), nbrs)

    def set_multigraph_rows(self, row_offsets, row_nbrs):
        row_offsets, row_nbrs = _np(row_offsets, np.uint64), _np(row_nbrs, np.uint32)
        self._rows_gen += 1
        self._ck(self.lib.gnnpe_set_multigraph_rows(self.ctx, len(row_offsets) - 1, _ptr(row_offsets, _u64p), _ptr(row_nbrs, _u32p)))

    def load_rows(self, n, labels, rows, row_offsets, row_nbrs, nbr_capacity=0):
        labels, rows = _np(labels, np.uint32), _np(rows, np.uint32)
        row_offsets, row_nbrs = _np(row_offsets, np.uint64), _np(row_nbrs, np.uint32)
        self._rows_gen += 1
        self.entries = 0
        self._ck(self.lib.gnnpe_load_rows(self.ctx, n, _ptr(labels, _u32p), len(rows), _ptr(rows, _u32p),
                                          _ptr(row_offsets, _u64p), _ptr(row_nbrs, _u32p), int(nbr_capacity)))
        self.n = n
        self.slab = (0, n)

    # R1: main.cpp:77-85
    def set_order(self, sorted_nodes, membership, p):
        sn, mem = _np(sorted_nodes, np.uint32), _np(membership, np.uint32)
        assert len(sn) == self.n and len(mem) == self.n
        self._ck(self.lib.gnnpe_set_order(self.ctx, _ptr(sn, _u32p), _ptr(mem, _u32p), int(p)))

    def set_slab(self, begin, end):
        self._ck(self.lib.gnnpe_set_slab(self.ctx, int(begin), int(end)))
        self.slab = (int(begin), int(end))

    # R3: gen_vde_x table (custom.h:492-511)
    def set_label_table(self, table):
        t = _np(table, np.float64)
        assert t.ndim == 2
        self._ck(self.lib.gnnpe_set_label_table(self.ctx, t.shape[0], t.shape[1], _ptr(t, _f64p)))
        self.e = t.shape[1]

    # R4: gen_vde (custom.h:513-544)
    def vde(self, want=True):
        if not want:
            self._ck(self.lib.gnnpe_vde(self.ctx, None, None, None))
            return None
        x = np.zeros((self.n, self.e))
        nx = np.zeros((self.n, self.e))
        v = np.zeros((self.n, self.e))
        self._ck(self.lib.gnnpe_vde(self.ctx, _ptr(x, _f64p), _ptr(nx, _f64p), _ptr(v, _f64p)))
        return x, nx, v

    def vde_device_ptr(self):
        a, b = _vp(), _vp()
        self._ck(self.lib.gnnpe_vde_device_ptr(self.ctx, C.byref(a), C.byref(b)))
        return a.value, b.value

    def vde_pack_slab(self, begin, end, dev_buf):
        self._ck(self.lib.gnnpe_vde_pack_slab(self.ctx, begin, end, _dev(dev_buf)))

    def vde_unpack_slab(self, begin, end, dev_buf):
        self._ck(self.lib.gnnpe_vde_unpack_slab(self.ctx, begin, end, _dev(dev_buf)))

    # R2: dfs + VectorHash (custom.h:52-92), count half
    def vde_unpack_all(self, bounds, stride, skip_rank, dev_buf):
        b = _np(bounds, np.uint32)
        self._ck(self.lib.gnnpe_vde_unpack_all(self.ctx, len(b) - 1, _ptr(b, _u32p), int(stride), int(skip_rank), _dev(dev_buf)))

    def count_paths(self, l=2, per_start=False):
        tot = C.c_uint64()
        ps = np.zeros(self.slab[1] - self.slab[0], np.uint64) if per_start else None
        self._ck(self.lib.gnnpe_count_paths(self.ctx, l, _ptr(ps, _u64p), C.byref(tot)))
        self.total = tot.value
        self.l = l
        return (tot.value, ps) if per_start else tot.value

    def count_paths_enqueue(self, l=2):
        """The count enqueued only (no read-back); count_total() fetches the number, count_total_device() copies it
        to a device word a collective can send."""
        self._ck(self.lib.gnnpe_count_paths_enqueue(self.ctx, l))
        self._total = None  # resolved by the first reader of .total (one read-back)
        self.l = l

    @property
    def total(self):
        """Paths of the last count; after an enqueue-only count the first read fetches it (count_total)."""
        if getattr(self, "_total", None) is None and getattr(self, "l", None) is not None:
            self.count_total()
        return getattr(self, "_total", None)

    @total.setter
    def total(self, value):
        self._total = value

    def count_total(self):
        tot = C.c_uint64()
        self._ck(self.lib.gnnpe_count_total(self.ctx, C.byref(tot)))
        self.total = tot.value
        return tot.value

    def count_total_device(self, dev_u64):
        self._ck(self.lib.gnnpe_count_total_device(self.ctx, _dev(dev_u64)))

    def fill_paths_capped_device(self, cap_rows, dev_vids=None, dev_pde=None):
        """Rows [0, min(total, cap_rows)) into buffers of cap_rows rows; the host never learns the total."""
        self._ck(self.lib.gnnpe_fill_paths_capped_device(self.ctx, int(cap_rows), _dev(dev_vids), _dev(dev_pde)))

    # R2 + R5: emit half (gen_pde, custom.h:546-572)
    def fill_paths(self, begin=0, end=None, ids=True, pde=True, pde_label=False, L=None):
        end = self.total if end is None else end
        cnt = end - begin
        L = getattr(self, "l", 2) + 1 if L is None else L
        D = self.e * L
        v = np.zeros((cnt, L), np.uint32) if ids else None
        p = np.zeros((cnt, D)) if pde else None
        q = np.zeros((cnt, D)) if pde_label else None
        self._ck(self.lib.gnnpe_fill_paths(self.ctx, begin, end, _ptr(v, _u32p), _ptr(p, _f64p), _ptr(q, _f64p)))
        return v, p, q

    def fill_paths_device(self, begin, end, dev_vids=None, dev_pde=None, dev_pde_label=None):
        self._ck(self.lib.gnnpe_fill_paths_device(self.ctx, begin, end, _dev(dev_vids), _dev(dev_pde),
                                                  _dev(dev_pde_label)))

    def rows_checksum_device(self, n_rows, L, dev_ids, first_id=0):
        out = C.c_uint64()
        self._ck(self.lib.gnnpe_rows_checksum_device(self.ctx, int(n_rows), int(L), _dev(dev_ids), int(first_id),
                                                     C.byref(out)))
        return out.value

    def set_degrees(self, degrees):
        d = _np(degrees, np.uint32)
        assert len(d) == self.n
        self._ck(self.lib.gnnpe_set_degrees(self.ctx, _ptr(d, _u32p)))

    # online filter (Partition::query, custom.h:366-489)
    def filter_candidates(self, plan, eps=1e-6):
        """plan: dict from host_query_plan.  Returns (bitmap [n_query_vertices x ceil(n/32)] uint32, device ms)."""
        nv = int(plan["n_vertices"])
        bm = np.zeros((nv, (self.n + 31) // 32), np.uint32)
        ms = C.c_double()
        v, l, d = (_np(plan[k], np.uint32) for k in ("vids", "labels", "degrees"))
        p = _np(plan["pde"], np.float64)
        self._ck(self.lib.gnnpe_filter_candidates(self.ctx, len(v), _ptr(v, _u32p), _ptr(l, _u32p), _ptr(d, _u32p),
                                                  _ptr(p, _f64p), nv, float(eps), _ptr(bm, _u32p), C.byref(ms)))
        return bm, ms.value

    def filter_candidates_exact(self, plan, eps=1e-6):
        """Exact-mode filter.  plan: dict from host_query_plan_exact (each path once: the library adds the reverses).
        Returns (bitmap [n_query_vertices x ceil(n/32)] uint32, device ms)."""
        l, counts, v, lb, d, pde, nv = self._exact_plan_args(plan)
        bm = np.zeros((nv, (self.n + 31) // 32), np.uint32)
        ms = C.c_double()
        self._ck(self.lib.gnnpe_filter_candidates_exact(self.ctx, l, counts, _ptr(v, _u32p), _ptr(lb, _u32p), _ptr(d, _u32p),
                                                        _ptr(pde, _f64p), nv, float(eps), _ptr(bm, _u32p), C.byref(ms)))
        return bm, ms.value

    @staticmethod
    def _exact_plan_args(plan):
        """the flat arrays of a plan dict from host_query_plan_exact, as the exact filter and the support calls take them"""
        parts = [plan[k] for k in ("main", "tri", "single")]
        counts = (C.c_uint32 * 3)(*[len(p["vids"]) for p in parts])
        v, lb, d = (np.ascontiguousarray(np.concatenate([np.asarray(p[k], np.uint32).ravel() for p in parts]))
                    for k in ("vids", "labels", "degrees"))
        pde = np.ascontiguousarray(np.concatenate([np.asarray(p["pde"], np.float64).ravel() for p in parts]))
        return int(plan["l"]), counts, v, lb, d, pde, int(plan["n_vertices"])

    def filter_support_exact(self, plan, eps=1e-6, table=None):
        """gnnpe_filter_support_exact: the support table S of the exact filter on the graph the context holds, (table, device ms).
        table[u, v] = the directed data paths (and single-vertex tests) that support bit v of row u of filter_candidates_exact,
        (n_query_vertices, n) uint64 held as int64 words on the device.  table: a torch device tensor, an object with data_ptr() or
        a device address to overwrite (it is returned as given); None allocates a torch tensor on the context's device.  Needs
        load_csr, the label table and vde() since the last change of the graph; no order."""
        l, counts, v, lb, d, pde, nv = self._exact_plan_args(plan)
        if table is None:
            import torch
            table = torch.zeros((nv, self.n), dtype=torch.int64, device=f"cuda:{self.device_index}")
            torch.cuda.synchronize(table.device)  # the library writes on the context's stream
        ms = C.c_double()
        self._ck(self.lib.gnnpe_filter_support_exact(self.ctx, l, counts, _ptr(v, _u32p), _ptr(lb, _u32p), _ptr(d, _u32p),
                                                     _ptr(pde, _f64p), nv, float(eps), _table_ptr(table), C.byref(ms)))
        return table, ms.value

    def filter_support_delta(self, plan, vertices, sign, table, eps=1e-6):
        """gnnpe_filter_support_exact_delta: table += sign * S_T with T = `vertices` (ids of the graph the context holds now, repeats
        tolerated; sign +1 or -1, mod 2^64): the support of the paths through T, each once.  An empty T launches nothing.  Around an
        update: subtract on the graph of before, update, vde(), add on the graph of after -- with T the ends of an edge batch,
        R and its neighbours for a relabel or a removal (include/gnnpe_hip.h).  Returns the device ms."""
        l, counts, v, lb, d, pde, nv = self._exact_plan_args(plan)
        t = _vertex_ids(vertices)
        ms = C.c_double()
        self._ck(self.lib.gnnpe_filter_support_exact_delta(self.ctx, l, counts, _ptr(v, _u32p), _ptr(lb, _u32p), _ptr(d, _u32p),
                                                           _ptr(pde, _f64p), nv, float(eps), _ptr(t, _u32p) if len(t) else None,
                                                           len(t), int(sign), _table_ptr(table), C.byref(ms)))
        return ms.value

    def filter_support_delta_device(self, plan, bits, ids, n_ids, sign, table, eps=1e-6):
        """gnnpe_filter_support_exact_delta_device: filter_support_delta with T taken from the device -- `bits` its bitmap
        (ceil(n / 32) uint32) and `ids` its n_ids ascending ids, as closed_neighbourhood and carry_vertex_set leave them (torch
        tensors, objects with data_ptr() or device addresses).  No sort, no upload of the list; for the same T the table's bytes
        are those of filter_support_delta.  Returns the device ms."""
        l, counts, v, lb, d, pde, nv = self._exact_plan_args(plan)
        ms = C.c_double()
        self._ck(self.lib.gnnpe_filter_support_exact_delta_device(self.ctx, l, counts, _ptr(v, _u32p), _ptr(lb, _u32p), _ptr(d, _u32p),
                                                                  _ptr(pde, _f64p), nv, float(eps), _table_ptr(bits), _table_ptr(ids),
                                                                  int(n_ids), int(sign), _table_ptr(table), C.byref(ms)))
        return ms.value

    def closed_neighbourhood(self, vertices, bits, ids, ids_cap=None, timing=False):
        """gnnpe_csr_closed_neighbourhood: T = R u N(R) of the graph on the device for R = `vertices` (repeats tolerated), written
        to the caller's device arrays `bits` (ceil(n / 32) uint32: every word, the bits at and above n zero) and `ids` (ascending,
        room for ids_cap of them: by default the length of a torch tensor).  Returns |T|, with the device ms appended with
        timing=True.  More than ids_cap vertices raise GnnpeError with the bitmap written; self.last_set_size holds |T| then."""
        r = _vertex_ids(vertices)
        return self._touched_call(lambda n, ms: self.lib.gnnpe_csr_closed_neighbourhood(
            self.ctx, _ptr(r, _u32p) if len(r) else None, len(r), _table_ptr(bits), _table_ptr(ids) if ids is not None else None,
            self._ids_cap(ids, ids_cap), n, ms), timing)

    def carry_vertex_set(self, bits_old, bits_new, ids, with_added=False, ids_cap=None, timing=False):
        """gnnpe_csr_carry_vertex_set: a vertex set of the graph before the last apply_vertices moved through its vertex map: bit
        v' of bits_new (ceil(n' / 32) uint32) is set where the old id of v' is in bits_old and, with with_added, where v' was
        added; `ids` receives the ascending ids.  Device arrays as closed_neighbourhood takes them; the same return value.
        Without a valid vertex map the call raises GnnpeError and launches nothing."""
        return self._touched_call(lambda n, ms: self.lib.gnnpe_csr_carry_vertex_set(
            self.ctx, _table_ptr(bits_old), 1 if with_added else 0, _table_ptr(bits_new), _table_ptr(ids) if ids is not None else None,
            self._ids_cap(ids, ids_cap), n, ms), timing)

    @staticmethod
    def _ids_cap(ids, ids_cap):
        if ids_cap is not None:
            return int(ids_cap)
        return int(ids.numel()) if hasattr(ids, "numel") else 0

    def _touched_call(self, call, timing):
        n, ms = C.c_uint64(), C.c_double()
        rc = call(C.byref(n), C.byref(ms) if timing else None)
        self.last_set_size = int(n.value)
        self._ck(rc)
        return (int(n.value), ms.value) if timing else int(n.value)

    def support_bitmap(self, table, n_query_vertices):
        """gnnpe_filter_support_bitmap: (bitmap, device ms), bit v of row u set where table[u, v] != 0 -- the candidate sets of
        filter_candidates_exact on the graph the table is current for, in the layout every refinement call takes."""
        bm = np.zeros((int(n_query_vertices), (self.n + 31) // 32), np.uint32)
        ms = C.c_double()
        self._ck(self.lib.gnnpe_filter_support_bitmap(self.ctx, int(n_query_vertices), _table_ptr(table), _ptr(bm, _u32p), C.byref(ms)))
        return bm, ms.value

    def refine(self, query_path, bitmap, limit=0xFFFFFFFF):
        """Refinement on the device (custom.h:634-932): (answers, device ms) from the filter's candidate bitmap."""
        out, ms = C.c_uint64(), C.c_double()
        bm = _np(bitmap, np.uint32)
        self._ck(load_online().gnnpe_refine(self.ctx, query_path.encode(), _ptr(bm, _u32p), int(limit), C.byref(out), C.byref(ms)))
        return out.value, ms.value

    def refine_sets(self, query_path, bitmap, limit=0xFFFFFFFF, matches_cap=0, distinct=False, induced=False):
        """Set-restricted refinement on the device (gnnpe_refine_sets): (answers, device ms), or with matches_cap > 0
        (answers, device ms, matches) -- matches[k, u] = image of query vertex u in the k-th embedding kept,
        min(answers, matches_cap) rows.  distinct=True: gnnpe_refine_sets_distinct, one embedding per distinct subgraph.
        induced=True: gnnpe_refine_sets_mode with GNNPE_MATCH_INDUCED, induced matches only."""
        out, ms = C.c_uint64(), C.c_double()
        bm = _np(bitmap, np.uint32)
        cap = min(int(matches_cap), int(limit))
        rows = None
        if matches_cap > 0:
            nq = bm.shape[0] if bm.ndim == 2 else bm.size // ((self.n + 31) // 32)
            rows = np.zeros((max(cap, 1), nq), np.uint32)
        if induced:
            self._ck(load_online().gnnpe_refine_sets_mode(self.ctx, query_path.encode(), _ptr(bm, _u32p), int(limit),
                                                          match_mode(distinct, induced), C.byref(out),
                                                          _ptr(rows, _u32p) if rows is not None else None, cap, C.byref(ms)))
        else:
            fn = load_online().gnnpe_refine_sets_distinct if distinct else load_online().gnnpe_refine_sets
            self._ck(fn(self.ctx, query_path.encode(), _ptr(bm, _u32p), int(limit), C.byref(out),
                        _ptr(rows, _u32p) if rows is not None else None, cap, C.byref(ms)))
        if rows is None:
            return out.value, ms.value
        return out.value, ms.value, rows[:min(out.value, cap)]

    def _sets_table(self, entry, shape, query_path, bitmap, limit, distinct, induced, device, edges=None, accum=None, sign=1):
        """One call of gnnpe_refine_sets_vertex_counts / _edge_counts or, where `edges` is given, of their _delta_ forms (which
        alone take accum and sign): (answers, complete, counts, device ms).  counts is the host table of `shape`, or with
        device=True or accum a view of the device table the call names."""
        out, done, ms, ptr = C.c_uint64(), C.c_int(), C.c_double(), C.c_void_p()
        bm = _np(bitmap, np.uint32)
        counts = None if device or accum is not None else np.zeros(shape, np.uint64)
        args = [self.ctx, query_path.encode(), _ptr(bm, _u32p)]
        if edges is not None:
            args += [_ptr(edges, _u32p) if len(edges) else None, len(edges)]
        args += [int(limit), match_mode(distinct, induced), C.byref(out), C.byref(done), _ptr(counts, _u64p), C.byref(ptr)]
        if edges is not None:
            args += [None if accum is None else C.c_void_p(int(accum)), int(sign)]
        self._ck(getattr(load_online(), entry)(*args, C.byref(ms)))
        if counts is None:
            counts = _DevArray(int(ptr.value or 0), shape, "<i8", owner=self)
        return out.value, bool(done.value), counts, ms.value

    def refine_sets_vertex_counts(self, query_path, bitmap, limit=2 ** 64 - 1, distinct=False, induced=False, device=False):
        """Per-vertex match counts on the device (gnnpe_refine_sets_vertex_counts): (answers, complete, counts, device ms) with
        counts[u, v] = the matches of the mode that send query vertex u to data vertex v, (nq, n) uint64.  `limit` is a guard:
        complete = matches < limit, and counts is exact only where complete.  device=True: counts is a view of the context's
        device table (`torch.as_tensor(counts, device=...)` shares it: int64 words holding the uint64 counts), with no host copy,
        valid until the next call of this method or until another graph is loaded."""
        bm = _np(bitmap, np.uint32)
        return self._sets_table("gnnpe_refine_sets_vertex_counts", (_bitmap_rows(bm, self.n), self.n), query_path, bm, limit, distinct,
                                induced, device)

    def refine_sets_edge_counts(self, query_path, bitmap, limit=2 ** 64 - 1, distinct=False, induced=False, device=False):
        """Per-edge match counts on the device (gnnpe_refine_sets_edge_counts): (answers, complete, counts, device ms) with
        counts[k, j] = the matches of the mode that send query edge k = host_query_edges(query_path)[k] onto adjacency entry j of
        the CSR given to load_csr, (nqe, entries) uint64.  `limit` is a guard: complete = matches < limit, and counts is exact only
        where complete.  device=True: counts is a view of the context's device table (`torch.as_tensor(counts, device=...)`
        shares it: int64 words holding the uint64 counts), with no host copy, valid until the next call of this method or until
        another graph is loaded; edge_counts_to_host(counts) copies it back and refuses a view that is no longer valid."""
        shape = (len(host_query_edges(query_path)), self.entries)
        self._ecounts_call += 1
        got = self._sets_table("gnnpe_refine_sets_edge_counts", shape, query_path, bitmap, limit, distinct, induced, device)
        if device:
            got[2].valid_for = (self._rows_gen, self._ecounts_call)
        return got

    def refine_sets_delta(self, query_path, bitmap, edges, limit=2 ** 64 - 1, matches_cap=0, distinct=False, induced=False):
        """The matches through a set of data edges on the device (gnnpe_refine_sets_delta): (answers, rows, device ms).  answers =
        min(limit, the matches of the mode that put at least one query edge on one of `edges`), each match once; rows[k, u] = the
        image of query vertex u in the k-th match kept, min(answers, matches_cap) rows (none with matches_cap 0).  `edges`: pairs
        (x, y) of the loaded graph, either orientation, repeats tolerated; a pair that is no edge is refused."""
        out, ms = C.c_uint64(), C.c_double()
        bm, e = _np(bitmap, np.uint32), _delta_pairs(edges)
        cap = min(int(matches_cap), int(limit))
        nq = _bitmap_rows(bm, self.n)
        rows = np.zeros((cap, nq), np.uint32)
        self._ck(load_online().gnnpe_refine_sets_delta(self.ctx, query_path.encode(), _ptr(bm, _u32p), _ptr(e, _u32p) if len(e) else None,
                                                       len(e), int(limit), match_mode(distinct, induced), C.byref(out),
                                                       _ptr(rows, _u32p) if cap else None, cap, C.byref(ms)))
        return out.value, rows[:min(out.value, cap)], ms.value

    def refine_sets_delta_vertices(self, query_path, bitmap, vertices, limit=2 ** 64 - 1, matches_cap=0, distinct=False, induced=False):
        """The matches through a set of data vertices on the device (gnnpe_refine_sets_delta_vertices): (answers, rows, device ms).
        answers = min(limit, the matches of the mode with at least one image among `vertices`), each match once; rows as
        refine_sets_delta's.  `vertices`: ids of the loaded graph, repeats tolerated; an id the graph does not have is refused."""
        out, ms = C.c_uint64(), C.c_double()
        bm, s = _np(bitmap, np.uint32), _vertex_ids(vertices)
        cap = min(int(matches_cap), int(limit))
        nq = _bitmap_rows(bm, self.n)
        rows = np.zeros((cap, nq), np.uint32)
        self._ck(load_online().gnnpe_refine_sets_delta_vertices(self.ctx, query_path.encode(), _ptr(bm, _u32p),
                                                                _ptr(s, _u32p) if len(s) else None, len(s), int(limit),
                                                                match_mode(distinct, induced), C.byref(out),
                                                                _ptr(rows, _u32p) if cap else None, cap, C.byref(ms)))
        return out.value, rows[:min(out.value, cap)], ms.value

    def refine_sets_delta_nonedges(self, query_path, bitmap, pairs, limit=2 ** 64 - 1, matches_cap=0, distinct=False):
        """The induced matches on a set of non-edges on the device (gnnpe_refine_sets_delta_nonedges): (answers, rows, device ms).
        answers = min(limit, the induced matches -- with distinct=True of the INDUCED | DISTINCT mode -- that put at least one
        non-adjacent query pair on one of `pairs`), each match once; rows as refine_sets_delta's.  `pairs`: (x, y) that are NOT
        edges of the loaded graph, either orientation, repeats tolerated; a pair that is an edge is refused."""
        out, ms = C.c_uint64(), C.c_double()
        bm, e = _np(bitmap, np.uint32), _delta_pairs(pairs)
        cap = min(int(matches_cap), int(limit))
        nq = _bitmap_rows(bm, self.n)
        rows = np.zeros((cap, nq), np.uint32)
        self._ck(load_online().gnnpe_refine_sets_delta_nonedges(self.ctx, query_path.encode(), _ptr(bm, _u32p),
                                                                _ptr(e, _u32p) if len(e) else None, len(e), int(limit),
                                                                match_mode(distinct, True), C.byref(out),
                                                                _ptr(rows, _u32p) if cap else None, cap, C.byref(ms)))
        return out.value, rows[:min(out.value, cap)], ms.value

    def _refine_sets_delta_counts(self, kind, shape, query_path, bitmap, edges, limit, distinct, induced, device, accum, sign):
        e = _vertex_ids(edges) if kind.startswith("vertices_") else _delta_pairs(edges)  # (S travels where F does)
        if accum is None:
            self._delta_counts_call[kind] += 1
        got = self._sets_table(f"gnnpe_refine_sets_delta_{kind}_counts", shape, query_path, bitmap, limit, distinct, induced, device, e,
                               accum, sign)
        if device and accum is None:
            got[2].valid_for = (kind, self._rows_gen, self._delta_counts_call[kind])
        return got

    def refine_sets_delta_vertex_counts(self, query_path, bitmap, edges, limit=2 ** 64 - 1, distinct=False, induced=False, device=False,
                                        accum=None, sign=1):
        """The per-vertex table of the matches through a set of data edges on the device (gnnpe_refine_sets_delta_vertex_counts):
        (answers, complete, counts, device ms) as refine_sets_vertex_counts, over the matches refine_sets_delta counts only.
        device=True: counts is a view of the context's own table for this call, valid until the next such call or until the rows
        are loaded or changed (apply_edges); delta_counts_to_host(counts) copies it back.  accum: a device pointer (an int, a
        tensor's data_ptr()) to the caller's (nq, n) uint64 table on the context's device: nothing is zeroed, every cell gets
        sign * its count added (sign +1 or -1, mod 2^64), counts is a view of the caller's memory, and a refused call leaves it
        untouched.  Pass the default limit when accumulating."""
        bm = _np(bitmap, np.uint32)
        return self._refine_sets_delta_counts("vertex", (_bitmap_rows(bm, self.n), self.n), query_path, bm, edges, limit, distinct,
                                              induced, device, accum, sign)

    def refine_sets_delta_edge_counts(self, query_path, bitmap, edges, limit=2 ** 64 - 1, distinct=False, induced=False, device=False,
                                      accum=None, sign=1):
        """The per-edge table of the matches through a set of data edges on the device (gnnpe_refine_sets_delta_edge_counts):
        (answers, complete, counts, device ms) as refine_sets_edge_counts, over the matches refine_sets_delta counts only; the
        columns are the adjacency entries of the graph the context holds now.  device, accum and sign as for
        refine_sets_delta_vertex_counts, the caller's table being (nqe, entries) uint64."""
        shape = (len(host_query_edges(query_path)), self.entries)
        return self._refine_sets_delta_counts("edge", shape, query_path, bitmap, edges, limit, distinct, induced, device, accum, sign)

    def refine_sets_delta_nonedges_vertex_counts(self, query_path, bitmap, pairs, limit=2 ** 64 - 1, distinct=False, device=False,
                                                 accum=None, sign=1):
        """The per-vertex table of the induced matches on a set of non-edges on the device
        (gnnpe_refine_sets_delta_nonedges_vertex_counts): (answers, complete, counts, device ms) as refine_sets_vertex_counts, over
        the matches refine_sets_delta_nonedges counts only (with distinct=True of the INDUCED | DISTINCT mode).  device, accum and
        sign exactly as for refine_sets_delta_vertex_counts: a device=True view is of the context's own table for this call, valid
        until the next such call or until the rows are loaded or changed (apply_edges), and delta_counts_to_host(counts) copies it
        back.  With refine_sets_delta_vertex_counts an induced table is maintained across apply_edges: -VN(G, I), apply, +VD(G', I)
        for an insertion, -VD(G, D), apply, +VN(G', D) for a deletion."""
        bm = _np(bitmap, np.uint32)
        return self._refine_sets_delta_counts("nonedges_vertex", (_bitmap_rows(bm, self.n), self.n), query_path, bm, pairs, limit,
                                              distinct, True, device, accum, sign)

    def refine_sets_delta_nonedges_edge_counts(self, query_path, bitmap, pairs, limit=2 ** 64 - 1, distinct=False, device=False,
                                               accum=None, sign=1):
        """The per-edge table of the induced matches on a set of non-edges on the device
        (gnnpe_refine_sets_delta_nonedges_edge_counts): (answers, complete, counts, device ms) as refine_sets_edge_counts -- the rows
        are the query edges, the columns the adjacency entries of the graph the context holds now -- over the matches
        refine_sets_delta_nonedges counts only.  device, accum and sign as for refine_sets_delta_nonedges_vertex_counts, the caller's
        table being (nqe, entries) uint64."""
        shape = (len(host_query_edges(query_path)), self.entries)
        return self._refine_sets_delta_counts("nonedges_edge", shape, query_path, bitmap, pairs, limit, distinct, True, device, accum, sign)

    def refine_sets_delta_vertices_vertex_counts(self, query_path, bitmap, vertices, limit=2 ** 64 - 1, distinct=False, induced=False,
                                                 device=False, accum=None, sign=1):
        """The per-vertex table of the matches through a set of data vertices on the device
        (gnnpe_refine_sets_delta_vertices_vertex_counts): (answers, complete, counts, device ms) as refine_sets_vertex_counts, over
        the matches refine_sets_delta_vertices counts only.  device, accum and sign exactly as for refine_sets_delta_vertex_counts:
        a device=True view is of the context's own table for this call, valid until the next such call or until the rows are
        loaded or changed, and delta_counts_to_host(counts) copies it back.  A table is maintained across a relabel by
        -VV(G, C, S), set_vertex_labels, +VV(G', C', S)."""
        bm = _np(bitmap, np.uint32)
        return self._refine_sets_delta_counts("vertices_vertex", (_bitmap_rows(bm, self.n), self.n), query_path, bm, vertices, limit,
                                              distinct, induced, device, accum, sign)

    def refine_sets_delta_vertices_edge_counts(self, query_path, bitmap, vertices, limit=2 ** 64 - 1, distinct=False, induced=False,
                                               device=False, accum=None, sign=1):
        """The per-edge table of the matches through a set of data vertices on the device
        (gnnpe_refine_sets_delta_vertices_edge_counts): (answers, complete, counts, device ms) as refine_sets_edge_counts, over the
        matches refine_sets_delta_vertices counts only.  device, accum and sign as for refine_sets_delta_vertices_vertex_counts, the
        caller's table being (nqe, entries) uint64; a single-vertex query has no table (a view of address 0 and no rows)."""
        shape = (len(host_query_edges(query_path)), self.entries)
        return self._refine_sets_delta_counts("vertices_edge", shape, query_path, bitmap, vertices, limit, distinct, induced, device, accum,
                                              sign)

    def _counts_view_to_host(self, view, stamp, stale):
        """a device table of this context copied to the host as uint64, unless its valid_for is not `stamp` any more"""
        if getattr(view, "owner", None) is not self or getattr(view, "valid_for", None) != stamp:
            raise GnnpeError(stale)
        nbytes = view.shape[0] * view.shape[1] * 8
        if nbytes == 0:
            return np.zeros(view.shape, np.uint64)
        return self.copy_to_host(view.__cuda_array_interface__["data"][0], nbytes).view(np.uint64).reshape(view.shape)

    def delta_counts_to_host(self, view):
        """the context's own device table a refine_sets_delta_vertex_counts / _edge_counts or refine_sets_delta_nonedges_vertex_counts
        / _edge_counts(..., device=True) call returned, copied to the host as uint64; a view from before the latest such call or from before the rows were loaded or changed is refused"""
        kind = (getattr(view, "valid_for", None) or (None,))[0]
        return self._counts_view_to_host(view, (kind, self._rows_gen, self._delta_counts_call.get(kind)),
                                         "stale delta-count view: the table was replaced by a later call or the graph was loaded or changed")

    def edge_counts_to_host(self, view):
        """the device table a refine_sets_edge_counts(..., device=True) call returned, copied to the host as uint64; a view from
        before the latest such call or from before the rows were loaded again is refused: the buffer holds something else by now"""
        return self._counts_view_to_host(view, (self._rows_gen, self._ecounts_call),
                                         "stale edge-count view: the table was replaced by a later refine_sets_edge_counts call or the graph was loaded again")

    def open_match_cursor(self, query_path, bitmap, page_rows, limit=2 ** 64 - 1, device=False, distinct=False, induced=False):
        """A MatchCursor over the embeddings gnnpe_refine_sets counts (gnnpe_refine_pages_open), or with distinct=True over the ones
        gnnpe_refine_sets_distinct counts; induced=True keeps the induced matches only (gnnpe_refine_pages_open_mode)."""
        return MatchCursor(self, query_path, bitmap, page_rows, limit=limit, device=device, distinct=distinct, induced=induced)

    def match_pages(self, query_path, bitmap, page_rows, limit=2 ** 64 - 1, device=False, distinct=False, induced=False):
        """Generator over the pages of a MatchCursor: every embedding inside the sets exactly once, up to `limit`, at most
        page_rows per page (an empty last page is not yielded).  The cursor is closed when the generator ends or is dropped."""
        cur = MatchCursor(self, query_path, bitmap, page_rows, limit=limit, device=device, distinct=distinct, induced=induced)
        try:
            done = False
            while not done:
                rows, done = cur.next()
                if rows.shape[0]:
                    yield rows
        finally:
            cur.close()

    def open_delta_cursor(self, query_path, bitmap, page_rows, *, edges=None, nonedges=None, vertices=None, limit=2 ** 64 - 1, device=False,
                          distinct=False, induced=False):
        """A MatchCursor over the delta matches: with `edges` the matches refine_sets_delta counts (gnnpe_refine_pages_open_delta),
        with `nonedges` the ones refine_sets_delta_nonedges counts (gnnpe_refine_pages_open_delta_nonedges; the mode is induced
        whatever `induced` says, as there), with `vertices` the ones refine_sets_delta_vertices counts
        (gnnpe_refine_pages_open_delta_vertices).  Exactly one of the three is given.  Every match comes out once across the
        pages; changing the graph invalidates the cursor, so a deletion's cursor is drained before the batch is applied and an
        insertion's is opened after it."""
        given = [(sfx, a) for sfx, a in (("", edges), ("_nonedges", nonedges), ("_vertices", vertices)) if a is not None]
        if len(given) != 1:
            raise GnnpeError("open_delta_cursor: exactly one of edges, nonedges and vertices must be given")
        sfx, a = given[0]
        ids = _vertex_ids(a) if sfx == "_vertices" else _delta_pairs(a)
        return MatchCursor(self, query_path, bitmap, page_rows, limit=limit, device=device, distinct=distinct,
                           induced=induced or sfx == "_nonedges", anchor=(sfx, ids))

    def delta_pages(self, query_path, bitmap, page_rows, *, edges=None, nonedges=None, vertices=None, limit=2 ** 64 - 1, device=False,
                    distinct=False, induced=False):
        """Generator over the pages of open_delta_cursor's cursor: every delta match exactly once, up to `limit`, at most page_rows
        per page (an empty last page is not yielded).  The cursor is closed when the generator ends or is dropped."""
        cur = self.open_delta_cursor(query_path, bitmap, page_rows, edges=edges, nonedges=nonedges, vertices=vertices, limit=limit,
                                     device=device, distinct=distinct, induced=induced)
        try:
            done = False
            while not done:
                rows, done = cur.next()
                if rows.shape[0]:
                    yield rows
        finally:
            cur.close()

    def path_partitions_device(self, begin, end, dev_part):
        self._ck(self.lib.gnnpe_path_partitions_device(self.ctx, begin, end, _dev(dev_part)))

    def set_fill_variant(self, v):
        self._ck(self.lib.gnnpe_set_fill_variant(self.ctx, int(v)))

    def set_emit_shape(self, shape):
        """0 = whatever gnnpe_emit_calibrate_device measured faster into the buffer (start-vertex waves where nothing was measured),
        1 = one wave per start vertex, one-shot in launch order (k_fill_ranked), 2 = one wave per output tile (k_fill_tiles), 3 = persistent waves taking
        tiles from ticket counters (k_fill_tickets: measured, never chosen -- it lives in diagnostic builds, `make DIAG=1`; the
        shipped library answers with the tile kernel), 4 = shape 1's kernel as a resident grid of three workgroups per CU with ticket counters.
        Graphs with hub rows always take the start-vertex kernel."""
        self._ck(self.lib.gnnpe_set_emit_shape(self.ctx, int(shape)))

    EMIT_SHAPES = (1, 2, 4)
    EMIT_SHAPE_NAMES = {1: "starts", 2: "tiles", 3: "tickets", 4: "starts_low"}
    EMIT_SHAPE_KERNELS = {1: "k_fill_ranked", 2: "k_fill_tiles", 3: "k_fill_tiles", 4: "k_fill_ranked"}

    def has_emit_shape(self, shape):
        return int(shape) in self.EMIT_SHAPES

    def emit_kernel_name(self):
        return self.lib.gnnpe_emit_kernel_name(self.ctx).decode()

    def emit_calibrate_device(self, dev_vids=None, dev_pde=None, rows_cap=None):
        """Times the emit shapes 1 (start-vertex waves, one-shot), 4 (the same kernel as a resident grid of three workgroups per CU) and 2 (output tiles) into these
        buffers and keeps the fastest for them: dict(starts_ms, starts_low_ms, tiles_ms, kept, kept_shape).  rows_cap = the
        buffers' capacity in rows (default: the tensors' first dimension)."""
        if rows_cap is None:
            t = dev_pde if dev_pde is not None else dev_vids
            rows_cap = int(t.shape[0]) if hasattr(t, "shape") else (1 << 62)
        ms, k = (C.c_float * 5)(), C.c_int()
        self._ck(self.lib.gnnpe_emit_calibrate_device(self.ctx, int(rows_cap), _dev(dev_vids), _dev(dev_pde), ms, C.byref(k)))
        return dict(starts_ms=ms[1], starts_low_ms=ms[4], tiles_ms=ms[2], kept=self.EMIT_SHAPE_NAMES[k.value], kept_shape=k.value)

    # halo exchange helpers
    def halo_need(self, slab_bounds, dev_ids, cap):
        b = _np(slab_bounds, np.uint32)
        counts = np.zeros(len(b) - 1, np.uint64)
        self._ck(self.lib.gnnpe_halo_need(self.ctx, len(b) - 1, _ptr(b, _u32p), _dev(dev_ids), int(cap),
                                          _ptr(counts, _u64p)))
        return counts

    def rows_degree(self, n_req, dev_ids, dev_deg):
        self._ck(self.lib.gnnpe_rows_degree(self.ctx, int(n_req), _dev(dev_ids), _dev(dev_deg)))

    def rows_pack(self, n_req, dev_ids, dev_out, cap):
        self._ck(self.lib.gnnpe_rows_pack(self.ctx, int(n_req), _dev(dev_ids), _dev(dev_out), int(cap)))

    def rows_append(self, n_rows, dev_ids, dev_deg, dev_nbrs, n_nbrs, min_rank=0):
        """min_rank > 0: entries ranked before that processing position are dropped (last-hop halo rows)."""
        self._ck(self.lib.gnnpe_rows_append(self.ctx, int(n_rows), _dev(dev_ids), _dev(dev_deg), _dev(dev_nbrs),
                                            int(n_nbrs), int(min_rank)))

    def rows_held(self):
        """(rows, neighbour entries, hub rows) on the device: own rows plus the installed (truncated) halo."""
        r, e, h = C.c_uint64(), C.c_uint64(), C.c_uint32()
        self._ck(self.lib.gnnpe_rows_held(self.ctx, C.byref(r), C.byref(e), C.byref(h)))
        return r.value, e.value, h.value

    def apply_edges(self, insert=None, delete=None, timing=False):
        """gnnpe_csr_apply_edges: the batch of edge insertions and deletions (pairs (x, y), either orientation, repeats tolerated)
        applied to the whole graph on the device; afterwards the context is as load_csr of the new graph's compact CSR leaves
        it.  Returns its entry count, (entries, device ms) with timing=True.  A refused batch raises GnnpeError and changes
        nothing; an empty batch does nothing."""
        ins, dele = _delta_pairs([] if insert is None else insert), _delta_pairs([] if delete is None else delete)
        after, ms = C.c_uint64(), C.c_double()
        self._map_call += 1  # the entry map of an earlier apply_edges_map is gone
        self._ck(self.lib.gnnpe_csr_apply_edges(self.ctx, _ptr(ins, _u32p) if len(ins) else None, len(ins),
                                                _ptr(dele, _u32p) if len(dele) else None, len(dele), C.byref(after),
                                                C.byref(ms) if timing else None))
        if len(ins) or len(dele):
            self._rows_gen += 1  # device views of the count tables are stale
            self.slab = (0, self.n)
        self.entries = after.value
        return (after.value, ms.value) if timing else after.value

    def standing_open(self, query_path, l=2, eps=1e-6, distinct=False, induced=False, rows_cap=0, bitmap=None):
        """gnnpe_standing_open: a StandingQuery on this context (at most 16).  bitmap=None: the exact filter at path length l keeps
        the candidate sets (needs the label table and vde()); a bitmap: gnnpe_standing_open_sets, the caller's sets, which must be
        sound for every graph the handle will see.  rows_cap: how many created and destroyed rows a batch keeps."""
        return StandingQuery(self, query_path, l, eps, match_mode(distinct, induced), rows_cap, bitmap)

    def standing_apply_edges(self, insert=None, delete=None, timing=False):
        """gnnpe_standing_apply_edges: apply_edges that carries every open StandingQuery through the batch (and runs vde()).  A
        refused batch raises GnnpeError and changes nothing, neither the graph nor a handle.  Returns the device ms with timing."""
        ins, dele = _delta_pairs([] if insert is None else insert), _delta_pairs([] if delete is None else delete)
        ms = C.c_double()
        self._map_call += 1
        self._ck(load_online().gnnpe_standing_apply_edges(self.ctx, _ptr(ins, _u32p) if len(ins) else None, len(ins),
                                                          _ptr(dele, _u32p) if len(dele) else None, len(dele),
                                                          C.byref(ms) if timing else None))
        if len(ins) or len(dele):
            self._rows_gen += 1
            self.slab = (0, self.n)
            self.entries = self.rows_held()[1]
        return ms.value if timing else None

    def standing_set_labels(self, vertices, labels, timing=False):
        """gnnpe_standing_set_labels: set_vertex_labels that carries every open StandingQuery through the relabel (and runs
        vde()): afterwards each handle reports the matches the new labels created and destroyed, its rows and the change lists of
        its kept tables.  Pairs that change nothing are dropped; if none is left neither the graph nor its generation changes.  A
        refused batch raises GnnpeError and changes nothing, neither the graph nor a handle.  Returns the device ms with timing."""
        v, lab = _vertex_ids(vertices), _vertex_ids(labels)
        if len(v) != len(lab):
            raise GnnpeError("standing_set_labels: one label per vertex expected")
        ms = C.c_double()
        live = [sq for sq in self._standing if sq.handle]
        gen = live[0].result()[5] if live else None  # (a stale handle is refused by the call below as well)
        self._ck(load_online().gnnpe_standing_set_labels(self.ctx, _ptr(v, _u32p) if len(v) else None, _ptr(lab, _u32p) if len(v) else None,
                                                         len(v), C.byref(ms) if timing else None))
        # a batch of nothing but no-ops leaves graph and generation alone: the caller's device views stay valid
        if len(v) and (gen is None or live[0].result()[5] != gen):
            self._rows_gen += 1  # device views of the count tables are stale where a label changed
            self.slab = (0, self.n)
        return ms.value if timing else None

    def standing_apply_vertices(self, remove=None, add_labels=None, timing=False):
        """gnnpe_standing_apply_vertices: apply_vertices that carries every open StandingQuery through the batch (and runs vde()).
        The destroyed rows are in the ids of the graph before, the created rows and the change lists in those of the graph after.
        A refused batch (a StandingQuery opened with a bitmap is one reason) raises GnnpeError and changes nothing.  Returns
        n_after, with the device ms appended with timing."""
        rem, add = _vertex_ids([] if remove is None else remove), _vertex_ids([] if add_labels is None else add_labels)
        n2, ms = C.c_uint32(), C.c_double()
        self._map_call += 1
        self._ck(load_online().gnnpe_standing_apply_vertices(self.ctx, _ptr(rem, _u32p) if len(rem) else None, len(rem),
                                                             _ptr(add, _u32p) if len(add) else None, len(add), C.byref(n2),
                                                             C.byref(ms) if timing else None))
        if len(rem) or len(add):
            self._rows_gen += 1
            self.total = None
        self.n = int(n2.value)
        self.slab = (0, self.n)
        self.entries = self.rows_held()[1]
        return (self.n, ms.value) if timing else self.n

    def apply_edges_map(self, insert=None, delete=None, timing=False):
        """gnnpe_csr_apply_edges_map: apply_edges that also leaves the batch's entry map on the device.  Returns (entries_before,
        entries_after, map_view), with the device ms appended with timing=True.  map_view is a view of the context's own uint32
        buffer, one word per adjacency entry of the new graph: the index of the same entry in the graph of before, NO_ENTRY for
        an inserted edge (`torch.as_tensor(map_view, device=...)` shares it: int32 words).  It is valid until the next
        apply_edges_map or apply_edges or until the rows are loaded; entry_map_to_host(map_view) copies it back and refuses a
        stale view.  A refused batch raises GnnpeError, changes nothing and leaves no map; an empty batch gives the identity map."""
        ins, dele = _delta_pairs([] if insert is None else insert), _delta_pairs([] if delete is None else delete)
        before, after, ms, ptr = C.c_uint64(), C.c_uint64(), C.c_double(), C.c_void_p()
        self._map_call += 1
        self._ck(self.lib.gnnpe_csr_apply_edges_map(self.ctx, _ptr(ins, _u32p) if len(ins) else None, len(ins),
                                                    _ptr(dele, _u32p) if len(dele) else None, len(dele), C.byref(before),
                                                    C.byref(after), C.byref(ptr), C.byref(ms) if timing else None))
        if len(ins) or len(dele):
            self._rows_gen += 1  # device views of the count tables are stale
            self.slab = (0, self.n)
        self.entries = after.value
        view = _DevArray(int(ptr.value or 0), (after.value,), "<u4", owner=self)
        view.valid_for = ("entry_map", self._rows_gen, self._map_call)
        return (before.value, after.value, view) + ((ms.value,) if timing else ())

    def entry_map_to_host(self, view):
        """the entry map an apply_edges_map call returned, copied to the host as uint32; a view from before the latest
        apply_edges_map / apply_edges or from before the rows were loaded is refused: the buffer holds something else by now"""
        if getattr(view, "owner", None) is not self or getattr(view, "valid_for", None) != ("entry_map", self._rows_gen, self._map_call):
            raise GnnpeError("stale entry-map view: the map was replaced by a later apply_edges_map call or the graph was loaded or changed")
        if view.shape[0] == 0:
            return np.zeros(0, np.uint32)
        return self.copy_to_host(view.__cuda_array_interface__["data"][0], view.shape[0] * 4).view(np.uint32)

    def carry_entries(self, src, dst, n_rows, elem_bytes=8, timing=False):
        """gnnpe_csr_carry_entries: a caller's per-entry table moved from the entries of the graph before the last apply_edges_map
        to those of the graph after it, on the device: dst[r, j'] = src[r, map[j']], 0 at an inserted edge.  src is (n_rows,
        entries_before), dst (n_rows, entries_after), row-major, cells of elem_bytes = 8 (the count tables) or 4; both are device
        pointers (an int, a tensor's data_ptr(), or an object with data_ptr()) on the context's device and must not overlap.
        Without a valid map (none made, a refused batch, apply_edges or a load since) the call raises GnnpeError and launches
        nothing.  Returns None, the device ms with timing=True."""
        ms = C.c_double()
        ptrs = [C.c_void_p(int(p.data_ptr()) if hasattr(p, "data_ptr") else int(p)) if p is not None else None for p in (src, dst)]
        self._ck(self.lib.gnnpe_csr_carry_entries(self.ctx, int(n_rows), int(elem_bytes), ptrs[0], ptrs[1], C.byref(ms) if timing else None))
        return ms.value if timing else None

    def table_fold(self, table, delta, cells, change_cells=None, change_deltas=None, cap=0, timing=False):
        """gnnpe_table_fold: table += delta (mod 2^64) and delta = 0 over `cells` uint64 cells, both device pointers (an int, a
        tensor, or an object with data_ptr()); the first `cap` pairs (cell, int64 delta) of the nonzero delta cells, ascending, go
        to the device arrays change_cells (uint64) / change_deltas (int64), which may be None only with cap == 0.  Returns the true
        number of nonzero delta cells, with the device ms appended with timing=True."""
        n, ms = C.c_uint64(), C.c_double()
        self._ck(self.lib.gnnpe_table_fold(self.ctx, _dev(table), _dev(delta), int(cells), _dev(change_cells), _dev(change_deltas),
                                           int(cap), C.byref(n), C.byref(ms) if timing else None))
        return (n.value, ms.value) if timing else n.value

    def edges_below(self, table, n_rows, threshold, pairs=None, cap=0, timing=False):
        """gnnpe_csr_edges_below: the undirected edges of the resident graph whose support in `table` (n_rows x entries uint64 on
        the device: an int, a tensor, or an object with data_ptr()) is below `threshold`; the first `cap` of them go to the device
        array `pairs` (cap x 2 uint32, ascending (x, y) with x < y), which may be None only with cap == 0.  Returns (n_selected,
        min_kept): the true number of selected edges and the smallest support among the others (2^64 - 1 without one); the device
        ms appended with timing=True."""
        n, low, ms = C.c_uint64(), C.c_uint64(), C.c_double()
        self._ck(self.lib.gnnpe_csr_edges_below(self.ctx, _dev(table), int(n_rows), int(threshold), _dev(pairs), int(cap), C.byref(n), C.byref(low),
                                                C.byref(ms) if timing else None))
        return (n.value, low.value, ms.value) if timing else (n.value, low.value)

    def apply_vertices(self, remove=None, add_labels=None, entry_map=False, timing=False):
        """gnnpe_csr_apply_vertices: the vertices of `remove` (ids of the graph on the device, repeats tolerated) leave with their
        edges, the survivors keep their order under new ids, one vertex per label of add_labels is appended with an empty row;
        afterwards the context is as load_csr of the new graph's compact CSR leaves it.  Returns (n_after, entries_before,
        entries_after, vertex_map_view, entry_map_view), with the device ms appended with timing=True.  The views are of the
        context's own uint32 buffers: vertex_map_view holds the old id of every new vertex (NO_VERTEX for an added one),
        entry_map_view (None without entry_map=True) the old index of every adjacency entry of the new graph; both are valid until
        the next apply_vertices or until the rows are loaded or changed (the entry map also until the next apply_edges[_map]);
        vertex_map_to_host / entry_map_to_host copy them back and refuse a stale view.  carry_vertices, and with entry_map=True
        carry_entries, move the caller's tables through them.  A refused batch raises GnnpeError, changes nothing and leaves no
        map; an empty batch changes nothing and gives identity maps."""
        rem, add = _vertex_ids([] if remove is None else remove), _vertex_ids([] if add_labels is None else add_labels)
        n2, before, after, ms, vptr, eptr = C.c_uint32(), C.c_uint64(), C.c_uint64(), C.c_double(), C.c_void_p(), C.c_void_p()
        self._map_call += 1  # the maps of an earlier batch are gone
        self._ck(self.lib.gnnpe_csr_apply_vertices(self.ctx, _ptr(rem, _u32p) if len(rem) else None, len(rem),
                                                   _ptr(add, _u32p) if len(add) else None, len(add), C.byref(n2), C.byref(before),
                                                   C.byref(after), C.byref(vptr), C.byref(eptr) if entry_map else None,
                                                   C.byref(ms) if timing else None))
        if len(rem) or len(add):
            self._rows_gen += 1  # device views of the count tables are stale
            self.total = None
        self.n = int(n2.value)
        self.entries = after.value
        self.slab = (0, self.n)
        vview = _DevArray(int(vptr.value or 0), (self.n,), "<u4", owner=self)
        vview.valid_for = ("vertex_map", self._rows_gen, self._map_call)
        eview = None
        if entry_map:
            eview = _DevArray(int(eptr.value or 0), (after.value,), "<u4", owner=self)
            eview.valid_for = ("entry_map", self._rows_gen, self._map_call)
        return (self.n, before.value, after.value, vview, eview) + ((ms.value,) if timing else ())

    def vertex_map_to_host(self, view):
        """the vertex map an apply_vertices call returned, copied to the host as uint32; a stale view is refused as
        entry_map_to_host refuses one"""
        if getattr(view, "owner", None) is not self or getattr(view, "valid_for", None) != ("vertex_map", self._rows_gen, self._map_call):
            raise GnnpeError("stale vertex-map view: the map was replaced by a later apply_vertices call or the graph was loaded or changed")
        return self.copy_to_host(view.__cuda_array_interface__["data"][0], view.shape[0] * 4).view(np.uint32)

    def carry_vertices(self, src, dst, n_rows, elem_bytes=8, timing=False):
        """gnnpe_csr_carry_vertices: a caller's per-vertex table moved from the vertices of the graph before the last
        apply_vertices to those of the graph after it, on the device: dst[r, v'] = src[r, vertex_map[v']], 0 at an added vertex.
        src is (n_rows, n_before), dst (n_rows, n_after), row-major, cells of elem_bytes = 8 (the count tables) or 4; device
        pointers as carry_entries takes them, not overlapping.  Without a valid vertex map (none made, a refused batch, the rows
        loaded or changed since -- apply_edges included) the call raises GnnpeError and launches nothing.  Returns None, the
        device ms with timing=True."""
        ms = C.c_double()
        ptrs = [C.c_void_p(int(p.data_ptr()) if hasattr(p, "data_ptr") else int(p)) if p is not None else None for p in (src, dst)]
        self._ck(self.lib.gnnpe_csr_carry_vertices(self.ctx, int(n_rows), int(elem_bytes), ptrs[0], ptrs[1], C.byref(ms) if timing else None))
        return ms.value if timing else None

    def set_vertex_labels(self, vertices, labels, timing=False):
        """gnnpe_set_vertex_labels: label(vertices[i]) = labels[i] on the whole graph on the device; afterwards the context is as
        load_csr of the same rows with the new labels leaves it (the rows, the reverse positions and the hub list are not
        rebuilt).  Returns None, the device ms with timing=True.  A refused call (an id outside the graph, one vertex with two
        labels) raises GnnpeError and changes nothing; an empty list does nothing."""
        v, lab = _vertex_ids(vertices), _vertex_ids(labels)
        if len(v) != len(lab):
            raise GnnpeError("set_vertex_labels: one label per vertex expected")
        ms = C.c_double()
        self._ck(self.lib.gnnpe_set_vertex_labels(self.ctx, _ptr(v, _u32p) if len(v) else None, _ptr(lab, _u32p) if len(v) else None,
                                                  len(v), C.byref(ms) if timing else None))
        if len(v):
            self._rows_gen += 1  # device views of the count tables and of the entry map are stale
            self.slab = (0, self.n)
        return ms.value if timing else None

    def download_labels(self):
        """gnnpe_labels_download: the labels of the whole graph the context holds, n uint32"""
        labels = np.zeros(self.n, np.uint32)
        self._ck(self.lib.gnnpe_labels_download(self.ctx, _ptr(labels, _u32p)))
        return labels

    def download_csr(self):
        """gnnpe_csr_download: (offsets, nbrs) of the whole graph the context holds, the arrays the edge-count tables index"""
        offsets, cnt = np.zeros(self.n + 1, np.uint32), C.c_uint64()
        nbrs = np.zeros(self.rows_held()[1], np.uint32)
        self._ck(self.lib.gnnpe_csr_download(self.ctx, _ptr(offsets, _u32p), _ptr(nbrs, _u32p), len(nbrs), C.byref(cnt)))
        return offsets, nbrs[:cnt.value]

    def rows_drop_halo(self):
        self._ck(self.lib.gnnpe_rows_drop_halo(self.ctx))

    # R7: text rendering (main.cpp:98-119)
    def text_paths(self, n_rows, L, dev_vids, dev_text=None, cap=0):
        nb = C.c_uint64()
        self._ck(self.lib.gnnpe_text_paths(self.ctx, int(n_rows), int(L), _dev(dev_vids), _dev(dev_text), int(cap),
                                           C.byref(nb)))
        return nb.value

    def text_ids(self, n, dev_ids, dev_text=None, cap=0):
        nb = C.c_uint64()
        self._ck(self.lib.gnnpe_text_ids(self.ctx, int(n), _dev(dev_ids), _dev(dev_text), int(cap), C.byref(nb)))
        return nb.value

    def select_partition(self, n, dev_part, pid, id_base, dev_ids):
        cnt = C.c_uint64()
        self._ck(self.lib.gnnpe_select_partition(self.ctx, int(n), _dev(dev_part), int(pid), int(id_base),
                                                 _dev(dev_ids), C.byref(cnt)))
        return cnt.value

    # R6: index.dat (custom.h:235-257)
    def build_index_device(self, cnt, L, dev_vids):
        img, nb = _vp(), C.c_uint64()
        hdr = (C.c_int32 * 8)()
        self._ck(self.lib.gnnpe_build_index_device(self.ctx, int(cnt), int(L), _dev(dev_vids), C.byref(img),
                                                   C.byref(nb), hdr))
        return img.value, nb.value, list(hdr)

    def build_index_partition_device(self, pid):
        """index.dat image of partition pid straight from the enumeration state (pair-major build when eligible)."""
        img, nb = _vp(), C.c_uint64()
        hdr = (C.c_int32 * 8)()
        self._ck(self.lib.gnnpe_build_index_partition_device(self.ctx, int(pid), C.byref(img), C.byref(nb), hdr))
        return img.value, nb.value, list(hdr)

    def build_box_index_device(self, cnt, dim, dev_boxes):
        """cnt x 2*dim doubles (lo0, hi0, lo1, hi1, ...) -> same image format (GNN-PGE/include/custom.h:171-177)."""
        img, nb = _vp(), C.c_uint64()
        hdr = (C.c_int32 * 8)()
        self._ck(self.lib.gnnpe_build_box_index_device(self.ctx, int(cnt), int(dim), _dev(dev_boxes), C.byref(img),
                                                       C.byref(nb), hdr))
        return img.value, nb.value, list(hdr)

    def build_index(self, pid, path):
        self._ck(self.lib.gnnpe_build_index(self.ctx, int(pid), path.encode()))

    def build_index_files(self, paths, aux_paths=None):
        """index.dat (and optionally aux_index.bin) of partitions 0..len(paths)-1, the index files written side by side."""
        arr = (C.c_char_p * len(paths))(*[p.encode() for p in paths])
        aux = None if aux_paths is None else (C.c_char_p * len(aux_paths))(*[p.encode() for p in aux_paths])
        self._ck(self.lib.gnnpe_build_index_files(self.ctx, len(paths), arr, aux))

    def build_index_partition_aux_device(self, pid, fetch=False):
        """index.dat image of partition pid AND its auxiliary index in one build (leaf rows by the leaf kernel).  Returns
        (image ptr, nbytes, hdr, key ptr, degrees ptr, label_mbr ptr, n_nodes); fetch=True returns host arrays instead of the
        three pointers."""
        img, nb = _vp(), C.c_uint64()
        hdr = (C.c_int32 * 8)()
        k, d, m = _vp(), _vp(), _vp()
        N = C.c_uint32()
        self._ck(self.lib.gnnpe_build_index_partition_aux_device(self.ctx, int(pid), C.byref(img), C.byref(nb), hdr, C.byref(k),
                                                                 C.byref(d), C.byref(m), C.byref(N)))
        if not fetch:
            return img.value, nb.value, list(hdr), k.value, d.value, m.value, N.value
        L, D, n = self.l + 1, (self.l + 1) * self.e, N.value
        key, deg, mbr = np.zeros(n), np.zeros((n, L), np.uint32), np.zeros((n, 2 * D))
        for host, dev in ((key, k), (deg, d), (mbr, m)):
            if host.nbytes:
                self._ck(self.lib.gnnpe_copy_to_host(self.ctx, host.ctypes.data_as(_vp), dev, host.nbytes))
        return img.value, nb.value, list(hdr), key, deg, mbr, n

    def aux_index_device_ptrs(self, dev_image, nbytes, cnt, L, dev_tuples):
        """The same pass, results left on the device: (key ptr, degrees ptr, label_mbr ptr, n_nodes, D) -- context-owned
        arrays, valid until the next call."""
        k, d, m = _vp(), _vp(), _vp()
        N, D = C.c_uint32(), C.c_uint32()
        self._ck(self.lib.gnnpe_aux_index_device(self.ctx, _dev(dev_image), int(nbytes), int(cnt), int(L), _dev(dev_tuples),
                                                 C.byref(k), C.byref(d), C.byref(m), C.byref(N), C.byref(D)))
        return k.value, d.value, m.value, N.value, D.value

    def aux_index_device(self, dev_image, nbytes, cnt, L, dev_tuples):
        """Partition::build_auxiliary_index (custom.h:268-364) over an index.dat image in device memory; dev_tuples =
        the partition's paths [cnt x L] in partition order.  Returns host copies: key[N], degrees[N x L], label_mbr[N x 2D]."""
        k, d, m = _vp(), _vp(), _vp()
        N, D = C.c_uint32(), C.c_uint32()
        self._ck(self.lib.gnnpe_aux_index_device(self.ctx, _dev(dev_image), int(nbytes), int(cnt), int(L), _dev(dev_tuples),
                                                 C.byref(k), C.byref(d), C.byref(m), C.byref(N), C.byref(D)))
        n, dim = N.value, D.value
        return dict(key=self.copy_to_host(k.value, n * 8).view(np.float64),
                    degrees=self.copy_to_host(d.value, n * L * 4).view(np.uint32).reshape(n, L),
                    label_mbr=self.copy_to_host(m.value, n * 2 * dim * 8).view(np.float64).reshape(n, 2 * dim), L=int(L), D=dim)

    def build_aux_index(self, pid, path):
        self._ck(self.lib.gnnpe_build_aux_index(self.ctx, int(pid), path.encode()))

    def copy_to_host(self, dev_ptr, nbytes):
        out = np.zeros(nbytes, np.uint8)
        self._ck(self.lib.gnnpe_copy_to_host(self.ctx, out.ctypes.data_as(_vp), C.c_void_p(dev_ptr), int(nbytes)))
        return out

    # GNN-PGE offline (GNN-PGE/src/main.cpp:91-195)
    def pge_groups(self):
        pg = np.zeros((self.n, 4 * self.e))
        plg = np.zeros((self.n, 4 * self.e))
        self._ck(self.lib.gnnpe_pge_groups(self.ctx, _ptr(pg, _f64p), _ptr(plg, _f64p)))
        return pg, plg

    def pge_groups_device(self):
        """The same computation left on the device: (path_group, path_label_group) device addresses."""
        self._ck(self.lib.gnnpe_pge_groups(self.ctx, None, None))
        a, b = _vp(), _vp()
        self._ck(self.lib.gnnpe_pge_device_ptr(self.ctx, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def pge_build_index(self, vertices, path):
        v = _np(vertices, np.uint32)
        self._ck(self.lib.gnnpe_pge_build_index(self.ctx, len(v), _ptr(v, _u32p), path.encode()))

    # GNN-PGE online filter (GNN-PGE/src/main.cpp:197-361, custom.h:327-374)
    def pge_set_groups(self, pg, plg):
        """Path groups read from data_vertices.bin instead of pge_groups(): n x 4e doubles each (after load_csr and
        set_label_table)."""
        a, b = _np(pg, np.float64), _np(plg, np.float64)
        assert a.size == b.size == self.n * 4 * self.e, (a.shape, b.shape, self.n, self.e)
        self._ck(self.lib.gnnpe_pge_set_groups(self.ctx, _ptr(a, _f64p), _ptr(b, _f64p)))

    def pge_filter_candidates(self, q):
        """q: dict from host_pge_query_groups (labels, degrees, pg, plg).  Returns (bitmap [n_query_vertices x ceil(n/32)]
        uint32, device ms), the layout of filter_candidates."""
        l, d = _np(q["labels"], np.uint32), _np(q["degrees"], np.uint32)
        pg, plg = _np(q["pg"], np.float64), _np(q["plg"], np.float64)
        nv = len(l)
        assert len(d) == nv and pg.size == plg.size == nv * 4 * self.e, (nv, pg.shape, plg.shape, self.e)
        bm = np.zeros((nv, (self.n + 31) // 32), np.uint32)
        ms = C.c_double()
        self._ck(self.lib.gnnpe_pge_filter_candidates(self.ctx, nv, _ptr(l, _u32p), _ptr(d, _u32p), _ptr(pg, _f64p),
                                                      _ptr(plg, _f64p), _ptr(bm, _u32p), C.byref(ms)))
        return bm, ms.value
