"""ctypes binding of the two C ABIs (include/madicp_hip.h, include/madicp_host.h).

This is plumbing for tests and bench.py; the product classes with the reference's names live in
mad_icp_amd.pybind.{pyvector,pymadtree,pymadicp,pypeline} (C++), which bind to the same ABI.
There is no CPU implementation behind any HIP entry point: without libmadicp_hip.so, or without a GPU,
the calls fail loudly.
"""
import ctypes as C
import os
import sys

import numpy as np

_PKG = os.path.dirname(os.path.abspath(__file__))

NODE_DTYPE = np.dtype([("mean", "<f8", (3,)), ("dir", "<f8", (3,)), ("right", "<i4"), ("leaf_id", "<i4"),
                       ("bbox0", "<f8")])
assert NODE_DTYPE.itemsize == 64

MAX_TREES = 128
MAX_BATCH = 64


class MadIcpError(RuntimeError):
    pass


class IcpParams(C.Structure):
    _fields_ = [("min_ball", C.c_double), ("rho_ker", C.c_double), ("b_ratio", C.c_double)]


class RecordLayoutC(C.Structure):
    """madicp_record_layout (include/madicp_hip.h)"""
    _fields_ = [("point_step", C.c_int32), ("off_x", C.c_int32), ("off_y", C.c_int32), ("off_z", C.c_int32), ("off_t", C.c_int32),
                ("t_type", C.c_int32)]


class RecordSourceC(C.Structure):
    """madicp_record_source (include/madicp_hip.h)"""
    _fields_ = [("data", C.c_void_p), ("n_records", C.c_int64), ("layout", RecordLayoutC), ("R", C.c_double * 9), ("t", C.c_double * 3),
                ("min_range", C.c_double), ("max_range", C.c_double), ("t_scale", C.c_double), ("t_offset", C.c_double),
                ("kitti_correction", C.c_int32), ("reserved", C.c_int32)]


class AttrFieldC(C.Structure):
    """madicp_attr_field (include/madicp_hip.h)"""
    _fields_ = [("offset", C.c_int32), ("type", C.c_int32)]


class MapAlignParams(C.Structure):
    """madicp_map_align_params (include/madicp_hip.h, include/madicp_host.h)"""
    _fields_ = [("reach", C.c_int), ("max_dist", C.c_double), ("rho", C.c_double), ("min_count", C.c_uint32), ("flat", C.c_double)]


_dp = C.POINTER(C.c_double)
_ip =C.POINTER(C.c_int)
_u8p = C.POINTER(C.c_uint8)
_u32p = C.POINTER(C.c_uint32)
_i32p = C.POINTER(C.c_int32)
_u64p = C.POINTER(C.c_uint64)
_i64p = C.POINTER(C.c_int64)

# madicp_host_allreduce_fn: int (*)(void* user, void* buf, int64_t count, int kind)
HOST_ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int)
REDUCE_SUM_F64, REDUCE_MAX_U8 = 0, 1

_hip = None
_host = None
_DIR_OVERRIDE = None  # set on the second instance of this module that measure_variant() makes
_measure_mod = None


def measure_variant():
    """This module a second time, bound to the MEASUREMENT build of the libraries (mad_icp_amd/_measure: the same sources with
    -DMADICP_MEASURE, built by _build.build_measure()): `capi.measure_variant().Context(0)` has include/madicp_hip_measure.h's
    timing / calibration / test aids, which the product library the default `capi` loads does not export.  Both can be used
    in one process (bench.py times the product and takes its roofline's launch times from the variant's identical kernels)."""
    global _measure_mod
    if _DIR_OVERRIDE is not None:
        return sys.modules[__name__]
    if os.environ.get("MADICP_NATIVE_DIR"):  # (a process already pointed at another build: that build is the variant)
        return sys.modules[__name__]
    if _measure_mod is None:
        import importlib.util

        from . import _build

        spec = importlib.util.spec_from_file_location(__name__ + "_measure", os.path.abspath(__file__),
                                                      submodule_search_locations=None)
        m = importlib.util.module_from_spec(spec)
        m.__package__ = __package__
        sys.modules[spec.name] = m
        spec.loader.exec_module(m)
        m._DIR_OVERRIDE = _build.MEASURE_DIR
        _measure_mod = m
    return _measure_mod


def _load(name):
    path = os.path.join(_DIR_OVERRIDE or os.environ.get("MADICP_NATIVE_DIR") or _PKG, name)  # (same variable as _build.OUT)
    if name == "libmadicp_hip.so" and os.environ.get("MADICP_HIP_LIB"):
        path = os.environ["MADICP_HIP_LIB"]  # an instrumented build of the same library (tools/stamps.py)
    if not os.path.exists(path):
        raise MadIcpError(f"{name} is not built (run `python -m mad_icp_amd._build`); there is no fallback path")
    return C.CDLL(path)


def hip_lib():
    global _hip
    if _hip is None:
        L = _load("libmadicp_hip.so")
        L.madicp_last_error.restype = C.c_char_p
        L.madicp_ctx_create.argtypes = [C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]
        L.madicp_ctx_destroy.argtypes = [C.c_void_p]
        L.madicp_ctx_synchronize.argtypes = [C.c_void_p]
        L.madicp_ctx_get_option.argtypes = [C.c_void_p, C.c_char_p, _i64p]
        L.madicp_ctx_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_int64]
        L.madicp_ctx_get_option.argtypes = [C.c_void_p, C.c_char_p, _i64p]
        L.madicp_tree_upload.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, _ip]
        L.madicp_tree_upload_trusted.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_double, _ip]
        L.madicp_tree_release.argtypes = [C.c_void_p, C.c_int]
        L.madicp_tree_download.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int32]
        L.madicp_tree_transform.argtypes = [C.c_void_p, C.c_int, _dp, _dp]
        L.madicp_nn_search.argtypes = [C.c_void_p, C.c_int, _dp, C.c_int64, _u32p, _u32p, _dp, _i32p]
        L.madicp_nn_search_device_enqueue.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p,
                                                      C.c_void_p, C.c_void_p, C.c_void_p]
        L.madicp_moving_upload.argtypes = [C.c_void_p, _dp, C.c_int32, _ip]
        L.madicp_moving_update.argtypes = [C.c_void_p, C.c_int, _dp, C.c_int32]
        L.madicp_moving_release.argtypes = [C.c_void_p, C.c_int]
        if hasattr(L, "madicp_moving_update_async"):
            L.madicp_moving_update_async.argtypes = [C.c_void_p, C.c_int, _dp, C.c_int32]
            L.madicp_icp_publish_enqueue.argtypes = [C.c_void_p, C.c_int, _ip]
            L.madicp_icp_publish_collect.argtypes = [C.c_void_p, C.c_int, C.c_int, _dp, _dp, _dp, _i32p, _u64p]
        L.madicp_stream_submit.argtypes = [C.c_void_p, _dp, C.c_int32, _ip, C.c_int, _dp, C.POINTER(IcpParams), C.c_int, _ip]
        L.madicp_stream_submit_tree.argtypes = [C.c_void_p, C.c_int, _ip, C.c_int, _dp, C.POINTER(IcpParams), C.c_int, _ip]
        L.madicp_stream_collect.argtypes = [C.c_void_p, C.c_int, _dp, _dp, _dp, _u8p, _i32p, _u64p]
        # include/madicp_hip_measure.h: only the measurement build exports these (measure_variant())
        if hasattr(L, "madicp_nn_time_descend"):
            L.madicp_nn_time_descend.argtypes = [C.c_void_p, C.c_int, _dp, C.c_int64, C.c_int, _dp, _u64p]
            L.madicp_debug_stream_copy.argtypes = [C.c_void_p, C.c_int64, C.c_int, _dp]
            L.madicp_icp_time_linearize.argtypes = [C.c_void_p, C.c_int, _ip, _ip, C.c_int, _dp, C.POINTER(IcpParams), C.c_int,
                                                    _dp, _u64p]
            L.madicp_icp_time_registration.argtypes = [C.c_void_p, C.c_int, _ip, _ip, C.c_int, _dp, C.POINTER(IcpParams), C.c_int,
                                                       C.c_int, _dp, _dp, _u64p, _u64p]
            L.madicp_debug_tree_build_points.argtypes = [C.c_void_p, _dp, C.c_int64]
        if hasattr(L, "madicp_debug_tree_rho"):
            L.madicp_debug_tree_rho.argtypes = [C.c_void_p, C.c_int, _dp]
        if hasattr(L, "madicp_debug_gather16"):  # (absent from an older build loaded through MADICP_HIP_LIB for an A/B)
            L.madicp_debug_gather16.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_uint64, C.c_int, _dp]
        L.madicp_icp_linearize.argtypes = [C.c_void_p, C.c_int, _ip, C.c_int, _dp, C.POINTER(IcpParams), _dp, _dp,
                                           _u32p, _u8p, _u64p]
        L.madicp_icp_register.argtypes = [C.c_void_p, C.c_int, _ip, C.c_int, _dp, C.POINTER(IcpParams), C.c_int, _dp,
                                          _dp, _u8p, _dp, _u64p]
        L.madicp_icp_register_batch.argtypes = [C.c_void_p, C.c_int, _ip, _ip, C.c_int, _dp, C.POINTER(IcpParams),
                                                C.c_int, _dp, _dp, _i32p, _u64p]
        L.madicp_icp_register_batch_enqueue.argtypes = [C.c_void_p, C.c_int, _ip, _ip, C.c_int, _dp,
                                                        C.POINTER(IcpParams), C.c_int]
        L.madicp_icp_fetch.argtypes = [C.c_void_p, C.c_int, _dp, _dp, _dp, _i32p, _u64p]
        L.madicp_icp_fetch_matched.argtypes = [C.c_void_p, C.c_int, _u8p, C.c_int32]
        L.madicp_cloud_upload.argtypes = [C.c_void_p, _dp, C.c_int64, _ip]
        L.madicp_cloud_release.argtypes = [C.c_void_p, C.c_int]
        L.madicp_cloud_size.argtypes = [C.c_void_p, C.c_int, _i64p]
        L.madicp_cloud_download.argtypes = [C.c_void_p, C.c_int, _dp, C.c_int64]
        L.madicp_cloud_ingest_f32.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.c_int64, C.c_int, C.c_double, C.c_double,
                                              C.c_int, _ip, _i64p]
        L.madicp_cloud_ingest_records.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(RecordLayoutC), C.c_double, C.c_double,
                                                  C.c_int, _dp, _ip, _i64p, _dp]
        L.madicp_cloud_ingest_sources.argtypes = [C.c_void_p, C.POINTER(RecordSourceC), C.c_int, _dp, _ip, _i64p, _i64p, _dp]
        L.madicp_cloud_stamps.argtypes = [C.c_void_p, C.c_int, _dp, C.c_int64]
        L.madicp_cloud_ingest_sources_attr.argtypes = [C.c_void_p, C.POINTER(RecordSourceC), C.c_int, C.POINTER(AttrFieldC), _dp, _ip, _i64p,
                                                       _i64p, _dp]
        L.madicp_cloud_set_attr.argtypes = [C.c_void_p, C.c_int, _u32p, C.c_int64]
        L.madicp_cloud_attr.argtypes = [C.c_void_p, C.c_int, _u32p, C.c_int64]
        L.madicp_cloud_export_f32_attr.argtypes = [C.c_void_p, C.c_int, _dp, _dp, C.c_double, C.POINTER(C.c_float), _u32p, C.c_int64, _i64p]
        L.madicp_map_create_attr.argtypes = [C.c_void_p, C.c_double, C.c_int64, C.c_int64, _ip]
        L.madicp_map_download_attr.argtypes = [C.c_void_p, C.c_int, C.c_int64, _u32p, C.c_int64, _i64p]
        L.madicp_cloud_export_f32.argtypes = [C.c_void_p, C.c_int, _dp, _dp, C.c_double, C.POINTER(C.c_float), C.c_int64, _i64p]
        L.madicp_map_create.argtypes = [C.c_void_p, C.c_double, C.c_int64, C.c_int64, _ip]
        L.madicp_map_insert_cloud.argtypes = [C.c_void_p, C.c_int, C.c_int, _dp, _dp, _i64p, _i64p]
        L.madicp_map_size.argtypes = [C.c_void_p, C.c_int, _i64p]
        L.madicp_map_download_f32.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.POINTER(C.c_float), C.c_int64, _i64p]
        L.madicp_map_clear.argtypes = [C.c_void_p, C.c_int]
        L.madicp_map_prune.argtypes = [C.c_void_p, C.c_int, _dp, C.c_double, C.c_int64, _i64p, _i64p, _i64p]
        L.madicp_map_clear_rays.argtypes = [C.c_void_p, C.c_int, C.c_int, _dp, _dp, _dp, C.c_double, C.c_int64, _i64p, _i64p, _i64p]
        L.madicp_map_release.argtypes = [C.c_void_p, C.c_int]
        L.madicp_map_query_cloud.argtypes = [C.c_void_p, C.c_int, C.c_int, _dp, _dp, C.c_int, C.c_double, _i32p, _dp, _u64p, _u32p, _u32p,
                                             C.c_int64, _u64p]
        L.madicp_map_register_cloud.argtypes = [C.c_void_p, C.c_int, C.c_int, _dp, _dp, C.POINTER(MapAlignParams), C.c_int, _dp, _dp, _dp,
                                                _u64p, _i32p, _dp, C.c_int64]
        L.madicp_map_track_removed.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.madicp_map_removed_count.argtypes = [C.c_void_p, C.c_int, _i64p]
        L.madicp_map_take_removed.argtypes = [C.c_void_p, C.c_int, _u64p, C.POINTER(C.c_float), _u32p, C.c_int64, _i64p]
        L.madicp_map_download_keys.argtypes = [C.c_void_p, C.c_int, C.c_int64, _u64p, C.c_int64, _i64p]
        L.madicp_map_download_rows.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.POINTER(C.c_float), _u64p, _u32p, C.c_int64, _i64p]
        L.madicp_map_create_ev.argtypes = [C.c_void_p, C.c_double, C.c_int64, C.c_int64, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, _ip]
        L.madicp_map_download_evidence.argtypes = [C.c_void_p, C.c_int, C.c_int64, _u32p, C.c_int64, _i64p]
        L.madicp_map_download_min_evidence.argtypes = [C.c_void_p, C.c_int, C.c_uint32, C.POINTER(C.c_float), _u64p, _u32p, _u32p, C.c_int64,
                                                       _i64p]
        L.madicp_map_create_mom.argtypes = [C.c_void_p, C.c_double, C.c_int64, C.c_int64, C.c_int, _u32p, C.c_uint32, _ip]
        L.madicp_map_download_moments.argtypes = [C.c_void_p, C.c_int, C.c_int64, _u64p, C.c_int64, _i64p]
        L.madicp_map_download_surfels.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.POINTER(C.c_float), C.POINTER(C.c_float),
                                                  C.POINTER(C.c_float), _u32p, C.c_int64, _i64p]
        L.madicp_cloud_deskew_own_stamps.argtypes = [C.c_void_p, C.c_int, _dp, C.c_double, _i32p]
        L.madicp_cloud_deskew.argtypes = [C.c_void_p, C.c_int, _dp, C.c_double, _i32p]
        L.madicp_cloud_deskew_stamped.argtypes = [C.c_void_p, C.c_int, _dp, C.c_int64, _dp, C.c_double, _i32p]
        L.madicp_tree_build.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_double, _ip, _i32p]
        L.madicp_tree_build_begin.argtypes = [C.c_void_p, _dp, C.c_int64, C.c_double, C.c_double]
        L.madicp_tree_build_end.argtypes = [C.c_void_p, _ip, _i32p]
        L.madicp_tree_build_cancel.argtypes = [C.c_void_p]
        L.madicp_tree_info.argtypes = [C.c_void_p, C.c_int, _i32p, _i32p]
        L.madicp_tree_build_stats.argtypes = [C.c_void_p, _i32p]
        L.madicp_comm_unique_id.argtypes = [_u8p]
        L.madicp_comm_init.argtypes = [C.c_void_p, _u8p, C.c_int, C.c_int]
        L.madicp_comm_destroy.argtypes = [C.c_void_p]
        L.madicp_comm_init_host.argtypes = [C.c_void_p, C.c_int, C.c_int, HOST_ALLREDUCE_FN, C.c_void_p]
        if hasattr(L, "madicp_p2p_export"):
            L.madicp_p2p_export.argtypes = [C.c_void_p, _u8p]
            L.madicp_p2p_attach.argtypes = [C.c_void_p, _u8p, C.c_int, C.c_int]
            L.madicp_p2p_detach.argtypes = [C.c_void_p]
        _hip = L
    return _hip


def host_lib():
    global _host
    if _host is None:
        L = _load("libmadicp_host.so")
        L.madicp_host_tree_build.restype = C.c_void_p
        L.madicp_host_tree_build.argtypes = [_dp, C.c_int64, C.c_double, C.c_double, C.c_int]
        L.madicp_host_tree_free.argtypes = [C.c_void_p]
        L.madicp_host_tree_num_nodes.restype = C.c_int32
        L.madicp_host_tree_num_nodes.argtypes = [C.c_void_p]
        L.madicp_host_tree_num_leaves.restype = C.c_int32
        L.madicp_host_tree_num_leaves.argtypes = [C.c_void_p]
        L.madicp_host_tree_nodes.restype = C.c_void_p
        L.madicp_host_tree_nodes.argtypes = [C.c_void_p]
        L.madicp_host_tree_leaf_nodes.restype = C.c_void_p
        L.madicp_host_tree_leaf_nodes.argtypes = [C.c_void_p]
        L.madicp_host_tree_leaf_means.argtypes = [C.c_void_p, _dp]
        L.madicp_host_tree_transform.argtypes = [C.c_void_p, _dp, _dp]
        L.madicp_host_gn_update.argtypes = [_dp, _dp, _dp]
        L.madicp_host_det_of_inverse6.restype = C.c_double
        L.madicp_host_det_of_inverse6.argtypes = [_dp]
        L.madicp_host_set_threads.argtypes = [C.c_int]
        L.madicp_host_tree_rho2.restype = C.c_double
        L.madicp_host_tree_rho2.argtypes = [C.c_void_p]
        L.madicp_host_debug_deskew.argtypes = [_dp, C.c_int64, _dp, _dp, C.c_double, C.c_int, _dp]
        L.madicp_host_deskew_stamped.argtypes = [_dp, _dp, C.c_int64, _dp, _dp, C.c_double, _dp, _i32p]
        L.madicp_host_debug_tree_points.restype = C.c_int64
        L.madicp_host_ingest_records.argtypes = [C.c_void_p, C.c_int64, C.POINTER(RecordLayoutC), C.c_double, C.c_double, C.c_int, _dp,
                                                 _dp, _dp, _i64p, _dp]
        L.madicp_host_ingest_sources.argtypes = [C.POINTER(RecordSourceC), C.c_int, _dp, _dp, _dp, _i64p, _i64p, _dp]
        L.madicp_host_cloud_export_f32.argtypes = [_dp, C.c_int64, _dp, _dp, C.c_double, C.POINTER(C.c_float), C.c_int64, _i64p]
        L.madicp_host_map_create.argtypes = [C.c_double, C.c_int64, C.c_int64, C.POINTER(C.c_void_p)]
        L.madicp_host_map_insert.argtypes = [C.c_void_p, _dp, C.c_int64, _dp, _dp, _i64p, _i64p]
        L.madicp_host_map_size.argtypes = [C.c_void_p, _i64p]
        L.madicp_host_map_download_f32.argtypes = [C.c_void_p, C.c_int64, C.POINTER(C.c_float), C.c_int64, _i64p]
        L.madicp_host_map_clear.argtypes = [C.c_void_p]
        L.madicp_host_map_prune.argtypes = [C.c_void_p, _dp, C.c_double, C.c_int64, _i64p, _i64p, _i64p]
        L.madicp_host_map_clear_rays.argtypes = [C.c_void_p, _dp, C.c_int64, _dp, _dp, _dp, C.c_double, C.c_int64, _i64p, _i64p, _i64p]
        L.madicp_host_ingest_sources_attr.argtypes = [C.POINTER(RecordSourceC), C.c_int, C.POINTER(AttrFieldC), _dp, _dp, _dp, _u32p, _i64p,
                                                      _i64p, _dp]
        L.madicp_host_cloud_export_f32_attr.argtypes = [_dp, _u32p, C.c_int64, _dp, _dp, C.c_double, C.POINTER(C.c_float), _u32p, C.c_int64,
                                                        _i64p]
        L.madicp_host_map_create_attr.argtypes = [C.c_double, C.c_int64, C.c_int64, C.POINTER(C.c_void_p)]
        L.madicp_host_map_insert_attr.argtypes = [C.c_void_p, _dp, _u32p, C.c_int64, _dp, _dp, _i64p, _i64p]
        L.madicp_host_map_download_attr.argtypes = [C.c_void_p, C.c_int64, _u32p, C.c_int64, _i64p]
        L.madicp_host_map_track_removed.argtypes = [C.c_void_p, C.c_int]
        L.madicp_host_map_removed_count.argtypes = [C.c_void_p, _i64p]
        L.madicp_host_map_take_removed.argtypes = [C.c_void_p, _u64p, C.POINTER(C.c_float), _u32p, C.c_int64, _i64p]
        L.madicp_host_map_download_keys.argtypes = [C.c_void_p, C.c_int64, _u64p, C.c_int64, _i64p]
        L.madicp_host_map_download_rows.argtypes = [C.c_void_p, C.c_int64, C.POINTER(C.c_float), _u64p, _u32p, C.c_int64, _i64p]
        L.madicp_host_map_create_ev.argtypes = [C.c_double, C.c_int64, C.c_int64, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32,
                                                C.POINTER(C.c_void_p)]
        L.madicp_host_map_download_evidence.argtypes = [C.c_void_p, C.c_int64, _u32p, C.c_int64, _i64p]
        L.madicp_host_map_download_min_evidence.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_float), _u64p, _u32p, _u32p, C.c_int64, _i64p]
        L.madicp_host_map_create_mom.argtypes = [C.c_double, C.c_int64, C.c_int64, C.c_int, _u32p, C.c_uint32, C.POINTER(C.c_void_p)]
        L.madicp_host_map_download_moments.argtypes = [C.c_void_p, C.c_int64, _u64p, C.c_int64, _i64p]
        L.madicp_host_map_download_surfels.argtypes = [C.c_void_p, C.c_int64, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float),
                                                       _u32p, C.c_int64, _i64p]
        L.madicp_host_map_query.argtypes = [C.c_void_p, _dp, C.c_int64, _dp, _dp, C.c_int, C.c_double, _i32p, _dp, _u64p, _u32p, _u32p,
                                            C.c_int64, _u64p]
        L.madicp_host_map_register.argtypes = [C.c_void_p, _dp, C.c_int64, _dp, _dp, C.POINTER(MapAlignParams), C.c_int, _dp, _dp, _dp, _u64p,
                                               _i32p, _dp, C.c_int64]
        L.madicp_host_map_destroy.restype = None
        L.madicp_host_map_destroy.argtypes = [C.c_void_p]
        L.madicp_host_debug_tree_points.argtypes = [_dp, C.c_int64, C.c_double, C.c_double, C.c_int]
        L.madicp_host_debug_partition.restype = C.c_int64
        L.madicp_host_debug_partition.argtypes = [_dp, C.c_int64, _dp, _dp, C.c_int]
        L.madicp_host_keyframe_owner.argtypes = [C.c_int64, C.c_int]
        L.madicp_host_device_ctx.restype = C.c_void_p
        L.madicp_host_device_ctx.argtypes = []
        L.madicp_host_debug_ledger_create.restype = C.c_void_p
        L.madicp_host_debug_ledger_create.argtypes = [C.c_int, C.c_int, C.c_int]
        L.madicp_host_debug_ledger_free.argtypes = [C.c_void_p]
        L.madicp_host_debug_ledger_promote.argtypes = [C.c_void_p, _i64p, _i64p]
        L.madicp_host_debug_ledger_window.restype = C.c_int64
        L.madicp_host_debug_ledger_window.argtypes = [C.c_void_p, _i64p, _u8p, C.c_int64]
        L.madicp_host_debug_ledger_num_local.restype = C.c_int64
        L.madicp_host_debug_ledger_num_local.argtypes = [C.c_void_p]
        _host = L
    return _host


def _aid(name):
    """an entry point of include/madicp_hip_measure.h: not in the product library"""
    f = getattr(hip_lib(), name, None)
    if f is None:
        raise MadIcpError(name + " is a measurement / test aid: the product library does not export it — use "
                          "mad_icp_amd.capi.measure_variant() (mad_icp_amd/_measure, built by _build.build_measure())")
    return f


def _check(rc):
    if rc != 0:
        raise MadIcpError(f"madicp error {rc}: {hip_lib().madicp_last_error().decode()}")


def _f64(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if shape is not None:
        a = a.reshape(shape)
    return a


def pose12(T):
    T = np.asarray(T, dtype=np.float64)
    if T.shape == (12,):
        return T.copy()
    return np.concatenate([T[:3, :3].reshape(-1), T[:3, 3]]).copy()


def pose44(x):
    T = np.eye(4)
    T[:3, :3] = np.asarray(x[:9]).reshape(3, 3)
    T[:3, 3] = x[9:12]
    return T


def gn_update(H, b, X12):
    """MADicp::updateState on joined adders (host): returns the updated pose (12,)."""
    H = _f64(H, (36,))
    b = _f64(b, (6,))
    X = _f64(X12, (12,)).copy()
    host_lib().madicp_host_gn_update(H.ctypes.data_as(_dp), b.ctypes.data_as(_dp), X.ctypes.data_as(_dp))
    return X


class HostTree:
    """Linear MAD-tree built on the host (include/madicp_host.h)."""

    def __init__(self, points, b_max, b_min, max_parallel_level=0):
        pts = _f64(points)
        if pts.ndim != 2 or pts.shape[1] != 3 or pts.shape[0] == 0:
            raise ValueError("points must be a non-empty (N,3) array")
        self._h = host_lib().madicp_host_tree_build(pts.ctypes.data_as(_dp), pts.shape[0], b_max, b_min,
                                                    max_parallel_level)
        if not self._h:
            raise MadIcpError("tree build failed")
        self.num_nodes = host_lib().madicp_host_tree_num_nodes(self._h)
        self.num_leaves = host_lib().madicp_host_tree_num_leaves(self._h)

    def __del__(self):
        if getattr(self, "_h", None):
            host_lib().madicp_host_tree_free(self._h)
            self._h = None

    @property
    def nodes(self):
        """numpy view (NODE_DTYPE) of the library-owned node array (the view keeps this object alive)."""
        ptr = host_lib().madicp_host_tree_nodes(self._h)
        buf = (C.c_char * (64 * self.num_nodes)).from_address(ptr)
        buf._owner = self  # the array's base keeps the tree (and so the memory) alive
        return np.frombuffer(buf, dtype=NODE_DTYPE)

    @property
    def leaf_nodes(self):
        ptr = host_lib().madicp_host_tree_leaf_nodes(self._h)
        buf = (C.c_char * (4 * self.num_leaves)).from_address(ptr)
        buf._owner = self
        return np.frombuffer(buf, dtype=np.int32)

    def leaf_means(self):
        out = np.empty((self.num_leaves, 3))
        host_lib().madicp_host_tree_leaf_means(self._h, out.ctypes.data_as(_dp))
        return out

    def transform(self, R, t):
        R = _f64(R, (9,))
        t = _f64(t, (3,))
        host_lib().madicp_host_tree_transform(self._h, R.ctypes.data_as(_dp), t.ctypes.data_as(_dp))

    @property
    def rho2(self):
        return host_lib().madicp_host_tree_rho2(self._h)


def host_tree_points(points, b_max, b_min, max_parallel_level=0):
    """The cloud as the host builder's construction leaves it (the reference's container after MADtree::build): every
    leaf's members in the order the splits produced, the leaf's first member overwritten by its representative."""
    pts = np.ascontiguousarray(points, dtype=np.float64).copy()
    nl = host_lib().madicp_host_debug_tree_points(pts.ctypes.data_as(_dp), pts.shape[0], float(b_max), float(b_min),
                                                  int(max_parallel_level))
    if nl < 0:
        raise MadIcpError("madicp_host_debug_tree_points: bad arguments")
    return pts, int(nl)


def host_keyframe_owner(k, world):
    """madicp_host_keyframe_owner: the C++ restatement of sharded.keyframe_owner (-1 on bad arguments)."""
    return int(host_lib().madicp_host_keyframe_owner(int(k), int(world)))


class KeyframeLedger:
    """The window bookkeeping of a (sharded) Pipeline on its own (csrc/host/keyframe_ledger.h), through the host library's test
    hooks: no device involved."""

    def __init__(self, rank, world, num_keyframes):
        self._h = host_lib().madicp_host_debug_ledger_create(int(rank), int(world), int(num_keyframes))
        if not self._h:
            raise ValueError("need 0 <= rank < world and num_keyframes >= 1")
        self.num_keyframes = int(num_keyframes)

    def __del__(self):
        if getattr(self, "_h", None):
            host_lib().madicp_host_debug_ledger_free(self._h)
            self._h = None

    def promote(self):
        """One promotion: (ordinal, this rank owns it, evicted ordinal or None)."""
        o, e = C.c_int64(-1), C.c_int64(-1)
        rc = host_lib().madicp_host_debug_ledger_promote(self._h, C.byref(o), C.byref(e))
        if rc < 0:
            raise MadIcpError("madicp_host_debug_ledger_promote: bad arguments")
        return o.value, bool(rc), (e.value if e.value >= 0 else None)

    def window(self):
        """(ordinals in the window, oldest first; whether this rank holds each one's tree)."""
        cap = self.num_keyframes + 1
        o, l = np.empty(cap, np.int64), np.empty(cap, np.uint8)
        n = host_lib().madicp_host_debug_ledger_window(self._h, o.ctypes.data_as(_i64p), l.ctypes.data_as(_u8p), cap)
        if n < 0 or n > cap:
            raise MadIcpError("madicp_host_debug_ledger_window: %d entries" % n)
        return o[:n].copy(), l[:n].astype(bool)

    def num_local(self):
        return int(host_lib().madicp_host_debug_ledger_num_local(self._h))


def host_deskew(points, T_prev, T_now, sensor_hz, route=0):
    """Pipeline::deskew on the host (csrc/host/deskew.h).  Returns (cloud in azimuth order, naive velocity (6,), used_parallel_order)."""
    pts = np.ascontiguousarray(points, dtype=np.float64).copy()
    vel = np.empty(6)
    a, b = pose12(T_prev), pose12(T_now)
    rc = host_lib().madicp_host_debug_deskew(pts.ctypes.data_as(_dp), pts.shape[0], a.ctypes.data_as(_dp), b.ctypes.data_as(_dp),
                                             float(sensor_hz), int(route), vel.ctypes.data_as(_dp))
    if rc < 0:
        raise MadIcpError("madicp_host_debug_deskew: bad arguments")
    return pts, vel, bool(rc)


def host_deskew_stamped(points, stamps, T_prev, T_now, sensor_hz):
    """deskew_cloud_stamped on the host (csrc/host/deskew.h): motion compensation from per-point timestamps in [0, 1].
    Returns (cloud in input order, naive velocity (6,), chunk of every point (n,) int32)."""
    pts = np.ascontiguousarray(points, dtype=np.float64).copy()
    st = np.ascontiguousarray(stamps, dtype=np.float64)
    if pts.ndim != 2 or pts.shape[1] != 3 or st.shape != (pts.shape[0],):
        raise ValueError("points must be (n, 3) and stamps (n,)")
    vel = np.empty(6)
    chunks = np.empty(pts.shape[0], np.int32)
    a, b = pose12(T_prev), pose12(T_now)
    rc = host_lib().madicp_host_deskew_stamped(pts.ctypes.data_as(_dp), st.ctypes.data_as(_dp), pts.shape[0], a.ctypes.data_as(_dp),
                                               b.ctypes.data_as(_dp), float(sensor_hz), vel.ctypes.data_as(_dp),
                                               chunks.ctypes.data_as(_i32p))
    if rc < 0:
        raise MadIcpError("madicp_host_deskew_stamped: bad arguments")
    return pts, vel, chunks


def _records_args(records, layout, time_field, t_range):
    """(array kept alive, n_records, RecordLayoutC, t_range pointer or None) of a records call: a 1-D structured array (layout
    read off its dtype by mad_icp_amd.records unless given) or an (n, point_step) uint8 array with an explicit layout.  The
    layout is NOT validated here when given explicitly: the native refusals are what the callers of this plumbing test."""
    from mad_icp_amd import records as _records

    r = np.ascontiguousarray(records)
    if layout is None:
        layout = _records.layout_of(r.dtype, time_field)
    lay = RecordLayoutC(*(int(v) for v in layout))
    n = r.shape[0]
    if r.nbytes != n * lay.point_step and 12 <= lay.point_step <= 256:
        raise ValueError("records hold %d bytes, the layout says %d x %d" % (r.nbytes, n, lay.point_step))
    tr = None if t_range is None else np.ascontiguousarray(t_range, dtype=np.float64).reshape(2)
    return r, n, lay, tr


def host_ingest_records(records, min_range, max_range, kitti_correction, layout=None, time_field=None, t_range=None):
    """madicp_host_ingest_records: the host twin of Context.cloud_ingest_records.  Returns (points (kept, 3) float64, stamps (kept,)
    float64 or None without a time field, (t0, t1))."""
    r, n, lay, tr = _records_args(records, layout, time_field, t_range)
    xyz, st = np.empty((max(n, 1), 3)), np.empty(max(n, 1))
    kept, rng = C.c_int64(0), np.empty(2)
    rc = host_lib().madicp_host_ingest_records(r.ctypes.data_as(C.c_void_p), n, C.byref(lay), float(min_range), float(max_range),
                                               int(bool(kitti_correction)), tr.ctypes.data_as(_dp) if tr is not None else None,
                                               xyz.ctypes.data_as(_dp), st.ctypes.data_as(_dp), C.byref(kept), rng.ctypes.data_as(_dp))
    if rc != 0:
        raise MadIcpError("madicp_host_ingest_records: bad arguments")
    k = kept.value
    return xyz[:k].copy(), (st[:k].copy() if lay.t_type != 0 else None), (float(rng[0]), float(rng[1]))


def _sources_args(sources, t_range):
    """(arrays kept alive, RecordSourceC array, total records, has a time field, t_range pointer or None) of a sources call.
    `sources`: mad_icp_amd.records.Source objects; a Source's layout is read off its dtype unless given, and like _records_args
    NOTHING is validated here — the native refusals are what the callers of this plumbing test."""
    from mad_icp_amd import records as _records

    alive, arr = [], (RecordSourceC * max(len(sources), 1))()
    for k, src in enumerate(sources):
        r = np.ascontiguousarray(src.records)
        layout = src.layout if src.layout is not None else _records.layout_of(r.dtype, src.time_field)
        T = np.eye(4) if src.sensor_to_base is None else np.asarray(src.sensor_to_base, dtype=np.float64)
        c = arr[k]
        c.data, c.n_records, c.layout = r.ctypes.data, r.shape[0], RecordLayoutC(*(int(v) for v in layout))
        c.R[:], c.t[:] = [float(v) for v in T[:3, :3].reshape(-1)], [float(v) for v in T[:3, 3]]
        c.min_range, c.max_range, c.t_scale, c.t_offset = float(src.min_range), float(src.max_range), float(src.time_scale), float(src.time_offset)
        c.kitti_correction, c.reserved = int(bool(src.kitti_correction)), 0
        alive.append(r)
    total = sum(int(a.shape[0]) for a in alive)
    timed = bool(sources) and arr[0].layout.t_type != 0
    tr = None if t_range is None else np.ascontiguousarray(t_range, dtype=np.float64).reshape(2)
    return alive, arr, total, timed, tr


def host_ingest_sources(sources, t_range=None):
    """madicp_host_ingest_sources: the host twin of Context.cloud_ingest_sources.  Returns (points (kept, 3) float64, stamps (kept,)
    float64 or None without a time field, (t0, t1), survivors per source)."""
    alive, arr, total, timed, tr = _sources_args(sources, t_range)
    xyz, st = np.empty((max(total, 1), 3)), np.empty(max(total, 1))
    kept, rng, per = C.c_int64(0), np.empty(2), np.zeros(max(len(sources), 1), np.int64)
    rc = host_lib().madicp_host_ingest_sources(arr, len(sources), tr.ctypes.data_as(_dp) if tr is not None else None,
                                               xyz.ctypes.data_as(_dp), st.ctypes.data_as(_dp), C.byref(kept), per.ctypes.data_as(_i64p),
                                               rng.ctypes.data_as(_dp))
    if rc != 0:
        raise MadIcpError("madicp_host_ingest_sources: bad arguments")
    k = kept.value
    return xyz[:k].copy(), (st[:k].copy() if timed else None), (float(rng[0]), float(rng[1])), [int(v) for v in per[:len(sources)]]


def _attr_fields(sources):
    """The AttrFieldC array of a sources call, or None when no source names an attribute.  A Source's `attribute` is a field name
    or an (offset, type code) pair (mad_icp_amd.records.resolve_attribute); a source WITHOUT one among sources with one travels as
    type 0, so that the native refusal ("an attribute in every source or in none") is what the caller meets.  Like _sources_args
    nothing else is validated here."""
    from mad_icp_amd import records as _records

    if not any(getattr(s, "attribute", None) is not None for s in sources):
        return None
    arr = (AttrFieldC * len(sources))()
    for k, src in enumerate(sources):
        if src.attribute is None:
            arr[k].offset, arr[k].type = 0, 0
        elif isinstance(src.attribute, str):
            arr[k].offset, arr[k].type = _records.resolve_attribute(src.records, src.attribute)[:2]
        else:
            arr[k].offset, arr[k].type = (int(v) for v in src.attribute)
    return arr


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.uint32).reshape(-1)


def host_ingest_sources_attr(sources, t_range=None):
    """madicp_host_ingest_sources_attr: the host twin of Context.cloud_ingest_sources_attr.  Returns (points, stamps or None,
    (t0, t1), survivors per source, words (kept,) uint32 or None when no source names an attribute)."""
    alive, arr, total, timed, tr = _sources_args(sources, t_range)
    fields = _attr_fields(sources)
    xyz, st, words = np.empty((max(total, 1), 3)), np.empty(max(total, 1)), np.empty(max(total, 1), np.uint32)
    kept, rng, per = C.c_int64(0), np.empty(2), np.zeros(max(len(sources), 1), np.int64)
    rc = host_lib().madicp_host_ingest_sources_attr(arr, len(sources), fields, tr.ctypes.data_as(_dp) if tr is not None else None,
                                                    xyz.ctypes.data_as(_dp), st.ctypes.data_as(_dp), words.ctypes.data_as(_u32p),
                                                    C.byref(kept), per.ctypes.data_as(_i64p), rng.ctypes.data_as(_dp))
    if rc != 0:
        raise MadIcpError("madicp_host_ingest_sources_attr: bad arguments")
    k = kept.value
    return (xyz[:k].copy(), (st[:k].copy() if timed else None), (float(rng[0]), float(rng[1])), [int(v) for v in per[:len(sources)]],
            (words[:k].copy() if fields is not None else None))


def host_cloud_export_f32_attr(xyz, attr, R, t, voxel):
    """madicp_host_cloud_export_f32_attr: host_cloud_export_f32 with the cloud's attribute column (n words).  Returns ((M, 3)
    float32 rows, (M,) uint32 words)."""
    a, w = _f64(xyz).reshape(-1, 3), _u32(attr)
    Rm, tv = _f64(R, (9,)), _f64(t, (3,))
    n = a.shape[0]
    if w.shape[0] != n:
        raise ValueError("one attribute word per point")
    out, ow, m = np.empty((max(n, 1), 3), np.float32), np.empty(max(n, 1), np.uint32), C.c_int64(0)
    rc = host_lib().madicp_host_cloud_export_f32_attr(a.ctypes.data_as(_dp), w.ctypes.data_as(_u32p), n, Rm.ctypes.data_as(_dp),
                                                      tv.ctypes.data_as(_dp), float(voxel), out.ctypes.data_as(C.POINTER(C.c_float)),
                                                      ow.ctypes.data_as(_u32p), n, C.byref(m))
    if rc != 0:
        raise MadIcpError("madicp_host_cloud_export_f32_attr: error %d (bad arguments)" % rc)
    return out[:m.value].copy(), ow[:m.value].copy()


def host_cloud_export_f32(xyz, R, t, voxel):
    """madicp_host_cloud_export_f32: the host twin of Context.cloud_export_f32.  xyz (n, 3) float64 through (R (3, 3), t (3,)) as
    float32 rows: every point (voxel = 0) or the lowest-index point of every voxel.  Returns (M, 3) float32."""
    a = _f64(xyz).reshape(-1, 3)
    Rm, tv = _f64(R, (9,)), _f64(t, (3,))
    n = a.shape[0]
    out, m = np.empty((max(n, 1), 3), np.float32), C.c_int64(0)
    rc = host_lib().madicp_host_cloud_export_f32(a.ctypes.data_as(_dp), n, Rm.ctypes.data_as(_dp), tv.ctypes.data_as(_dp), float(voxel),
                                                 out.ctypes.data_as(C.POINTER(C.c_float)), n, C.byref(m))
    if rc != 0:
        raise MadIcpError("madicp_host_cloud_export_f32: error %d (bad arguments)" % rc)
    return out[:m.value].copy()


def _host_map_check(rc, what):
    if rc != 0:
        raise MadIcpError("%s: error %d (%s)" % (what, rc, "capacity" if rc == -4 else "bad arguments"))


def host_map_create(voxel, initial_rows, max_rows):
    """madicp_host_map_create: the host twin of Context.map_create.  Returns the handle the other host_map_* calls take;
    host_map_destroy frees it."""
    h = C.c_void_p()
    _host_map_check(host_lib().madicp_host_map_create(float(voxel), int(initial_rows), int(max_rows), C.byref(h)), "madicp_host_map_create")
    return h


def host_map_create_attr(voxel, initial_rows, max_rows):
    """madicp_host_map_create_attr: a host map with the attribute column (the twin of Context.map_create_attr)."""
    h = C.c_void_p()
    _host_map_check(host_lib().madicp_host_map_create_attr(float(voxel), int(initial_rows), int(max_rows), C.byref(h)),
                    "madicp_host_map_create_attr")
    return h


def host_map_insert_attr(h, xyz, attr, R, t):
    """host_map_insert with the cloud's attribute column (n words, or None: the cloud carries none)."""
    a = _f64(xyz).reshape(-1, 3)
    w = None if attr is None else _u32(attr)
    if w is not None and w.shape[0] != a.shape[0]:
        raise ValueError("one attribute word per point")
    Rm, tv = _f64(R, (9,)), _f64(t, (3,))
    added, rows = C.c_int64(0), C.c_int64(0)
    _host_map_check(host_lib().madicp_host_map_insert_attr(h, a.ctypes.data_as(_dp), w.ctypes.data_as(_u32p) if w is not None else None,
                                                           a.shape[0], Rm.ctypes.data_as(_dp), tv.ctypes.data_as(_dp), C.byref(added),
                                                           C.byref(rows)), "madicp_host_map_insert_attr")
    return added.value, rows.value


def host_map_download_attr(h, first_row=0):
    """The attribute words of rows [first_row, size) as (M - first_row,) uint32; MadIcpError on a map made without the column."""
    m = max(host_map_size(h) - int(first_row), 0)
    out, got = np.empty(max(m, 1), np.uint32), C.c_int64(0)
    _host_map_check(host_lib().madicp_host_map_download_attr(h, int(first_row), out.ctypes.data_as(_u32p), m, C.byref(got)),
                    "madicp_host_map_download_attr")
    return out[:got.value].copy()


def host_map_insert(h, xyz, R, t):
    """Folds xyz (n, 3) float64 through (R (3, 3), t (3,)) into the map.  Returns (rows added, rows the map holds)."""
    a = _f64(xyz).reshape(-1, 3)
    Rm, tv = _f64(R, (9,)), _f64(t, (3,))
    added, rows = C.c_int64(0), C.c_int64(0)
    _host_map_check(host_lib().madicp_host_map_insert(h, a.ctypes.data_as(_dp), a.shape[0], Rm.ctypes.data_as(_dp), tv.ctypes.data_as(_dp),
                                                      C.byref(added), C.byref(rows)), "madicp_host_map_insert")
    return added.value, rows.value


def host_map_size(h):
    rows = C.c_int64(0)
    _host_map_check(host_lib().madicp_host_map_size(h, C.byref(rows)), "madicp_host_map_size")
    return rows.value


def host_map_download_f32(h, first_row=0):
    """Rows [first_row, size) of the map as (M - first_row, 3) float32."""
    m = max(host_map_size(h) - int(first_row), 0)
    out, got = np.empty((max(m, 1), 3), np.float32), C.c_int64(0)
    _host_map_check(host_lib().madicp_host_map_download_f32(h, int(first_row), out.ctypes.data_as(C.POINTER(C.c_float)), m, C.byref(got)),
                    "madicp_host_map_download_f32")
    return out[:got.value].copy()


def host_map_prune(h, center, radius, watermark=0):
    """madicp_host_map_prune: the host twin of Context.map_prune.  Returns (rows removed, rows the map holds, the kept rows among
    rows [0, watermark))."""
    c = _f64(center, (3,))
    removed, rows, mark = C.c_int64(0), C.c_int64(0), C.c_int64(0)
    _host_map_check(host_lib().madicp_host_map_prune(h, c.ctypes.data_as(_dp), float(radius), int(watermark), C.byref(removed),
                                                     C.byref(rows), C.byref(mark)), "madicp_host_map_prune")
    return removed.value, rows.value, mark.value


def host_map_clear_rays(h, xyz, R, t, origin=(0.0, 0.0, 0.0), margin=0.0, watermark=0):
    """madicp_host_map_clear_rays: the host twin of Context.map_clear_rays over xyz (n, 3) float64.  Returns (rows removed, rows
    the map holds, the kept rows among rows [0, watermark))."""
    a = _f64(xyz).reshape(-1, 3)
    Rm, tv, o = _f64(R, (9,)), _f64(t, (3,)), _f64(origin, (3,))
    removed, rows, mark = C.c_int64(0), C.c_int64(0), C.c_int64(0)
    _host_map_check(host_lib().madicp_host_map_clear_rays(h, a.ctypes.data_as(_dp), a.shape[0], Rm.ctypes.data_as(_dp), tv.ctypes.data_as(_dp),
                                                          o.ctypes.data_as(_dp), float(margin), int(watermark), C.byref(removed),
                                                          C.byref(rows), C.byref(mark)), "madicp_host_map_clear_rays")
    return removed.value, rows.value, mark.value


def _query_buffers(n, per_point, with_keys, with_attr, with_ev):
    """the per-point buffers of a map query, in the C call's order (None: not asked for), and their ctypes arguments"""
    m = max(n, 1)
    bufs = [np.empty(m, np.int32) if per_point else None, np.empty(m, np.float64) if per_point else None,
            np.empty(m, np.uint64) if with_keys else None, np.empty(m, np.uint32) if with_attr else None,
            np.empty(m, np.uint32) if with_ev else None]
    args = [b.ctypes.data_as(ct) if b is not None else None for b, ct in zip(bufs, (_i32p, _dp, _u64p, _u32p, _u32p))]
    return bufs, args


def _query_answer(counts, bufs, n, per_point):
    c = tuple(int(v) for v in counts)
    return (c,) + tuple(b[:n].copy() for b in bufs if b is not None) if per_point else c


def host_map_query(h, xyz, R, t, reach=1, max_dist=float("inf"), per_point=True, with_keys=False, with_attr=False, with_ev=False):
    """madicp_host_map_query: the host twin of Context.map_query over xyz (n, 3) float64, the same answer bit for bit."""
    a = _f64(xyz).reshape(-1, 3)
    Rm, tv = _f64(R, (9,)), _f64(t, (3,))
    n = a.shape[0]
    bufs, args = _query_buffers(n, per_point, with_keys, with_attr, with_ev)
    counts = np.zeros(3, np.uint64)
    _host_map_check(host_lib().madicp_host_map_query(h, a.ctypes.data_as(_dp), n, Rm.ctypes.data_as(_dp), tv.ctypes.data_as(_dp), int(reach),
                                                     float(max_dist), *args, n, counts.ctypes.data_as(_u64p)), "madicp_host_map_query")
    return _query_answer(counts, bufs, n, per_point)


def _align_call(call, n, R, t, iterations, reach, max_dist, rho, min_count, flat, per_point):
    """the buffers of a map registration around `call(Rp, tp, params, iterations, out_R, out_t, trace, counts, row, e, capacity)`, and
    its answer: dict(R (3, 3), t (3,), X (K + 1, 12), H (K + 1, 6, 6), b (K + 1, 6), chi2 (K + 1,), counts (K + 1, 4) uint64
    [, row (n,) int32, e (n,) float64]) — row k the linearisation at X[k], the last one at the returned pose"""
    Rm, tv = _f64(R, (9,)), _f64(t, (3,))
    k1 = max(int(iterations), 0) + 1
    params = MapAlignParams(int(reach), float(max_dist), float(rho), int(min_count), float(flat))
    out_R, out_t = np.zeros(9), np.zeros(3)
    trace, counts = np.zeros((k1, 40)), np.zeros((k1, 4), np.uint64)
    row = np.empty(max(n, 1), np.int32) if per_point else None
    e = np.empty(max(n, 1), np.float64) if per_point else None
    call(Rm.ctypes.data_as(_dp), tv.ctypes.data_as(_dp), C.byref(params), int(iterations), out_R.ctypes.data_as(_dp),
         out_t.ctypes.data_as(_dp), trace.ctypes.data_as(_dp), counts.ctypes.data_as(_u64p),
         row.ctypes.data_as(_i32p) if per_point else None, e.ctypes.data_as(_dp) if per_point else None, n)
    H = np.zeros((k1, 6, 6))
    v = 12
    for c in range(6):
        for r in range(c, 6):
            H[:, r, c] = H[:, c, r] = trace[:, v]
            v += 1
    ans = dict(R=out_R.reshape(3, 3), t=out_t, X=trace[:, :12].copy(), H=H, b=trace[:, 33:39].copy(), chi2=trace[:, 39].copy(), counts=counts)
    if per_point:
        ans["row"], ans["e"] = row[:n].copy(), e[:n].copy()
    return ans


def host_map_register(h, xyz, R, t, iterations, reach=1, max_dist=float("inf"), rho=float("inf"), min_count=3, flat=1.0, per_point=False):
    """madicp_host_map_register: the host twin of Context.map_register_cloud over xyz (n, 3) float64."""
    a = _f64(xyz).reshape(-1, 3)
    n = a.shape[0]

    def call(*args):
        _host_map_check(host_lib().madicp_host_map_register(h, a.ctypes.data_as(_dp) if n else None, n, *args), "madicp_host_map_register")

    return _align_call(call, n, R, t, iterations, reach, max_dist, rho, min_count, flat, per_point)


def host_map_track_removed(h, on=True):
    """madicp_host_map_track_removed: the host twin of Context.map_track_removed."""
    _host_map_check(host_lib().madicp_host_map_track_removed(h, 1 if on else 0), "madicp_host_map_track_removed")


def host_map_removed_count(h):
    n = C.c_int64(0)
    _host_map_check(host_lib().madicp_host_map_removed_count(h, C.byref(n)), "madicp_host_map_removed_count")
    return n.value


def host_map_take_removed(h, with_attr=False):
    """madicp_host_map_take_removed: the host twin of Context.map_take_removed.  Returns (keys (n,) uint64, rows (n, 3) float32
    [, words (n,) uint32]) and empties the log."""
    n = host_map_removed_count(h)
    keys, xyz, got = np.empty(max(n, 1), np.uint64), np.empty((max(n, 1), 3), np.float32), C.c_int64(0)
    w = np.empty(max(n, 1), np.uint32) if with_attr else None
    _host_map_check(host_lib().madicp_host_map_take_removed(h, keys.ctypes.data_as(_u64p), xyz.ctypes.data_as(C.POINTER(C.c_float)),
                                                            w.ctypes.data_as(_u32p) if with_attr else None, n, C.byref(got)),
                    "madicp_host_map_take_removed")
    m = got.value
    return (keys[:m].copy(), xyz[:m].copy()) + ((w[:m].copy(),) if with_attr else ())


def host_map_download_keys(h, first_row=0):
    """The stored voxel keys of rows [first_row, size) as (M - first_row,) uint64."""
    m = max(host_map_size(h) - int(first_row), 0)
    out, got = np.empty(max(m, 1), np.uint64), C.c_int64(0)
    _host_map_check(host_lib().madicp_host_map_download_keys(h, int(first_row), out.ctypes.data_as(_u64p), m, C.byref(got)),
                    "madicp_host_map_download_keys")
    return out[:got.value].copy()


def host_map_download_rows(h, first_row=0, with_keys=True, with_attr=False):
    """madicp_host_map_download_rows: the columns of rows [first_row, size): (rows (M, 3) float32[, keys uint64][, words uint32])."""
    m = max(host_map_size(h) - int(first_row), 0)
    xyz, got = np.empty((max(m, 1), 3), np.float32), C.c_int64(0)
    k = np.empty(max(m, 1), np.uint64) if with_keys else None
    w = np.empty(max(m, 1), np.uint32) if with_attr else None
    _host_map_check(host_lib().madicp_host_map_download_rows(h, int(first_row), xyz.ctypes.data_as(C.POINTER(C.c_float)),
                                                             k.ctypes.data_as(_u64p) if with_keys else None,
                                                             w.ctypes.data_as(_u32p) if with_attr else None, m, C.byref(got)),
                    "madicp_host_map_download_rows")
    g = got.value
    return (xyz[:g].copy(),) + ((k[:g].copy(),) if with_keys else ()) + ((w[:g].copy(),) if with_attr else ())


def host_map_create_ev(voxel, initial_rows, max_rows, hit, miss, cap, with_attr=False):
    """madicp_host_map_create_ev: a host map with the evidence column (the twin of Context.map_create_ev)."""
    h = C.c_void_p()
    _host_map_check(host_lib().madicp_host_map_create_ev(float(voxel), int(initial_rows), int(max_rows), 1 if with_attr else 0, int(hit),
                                                         int(miss), int(cap), C.byref(h)), "madicp_host_map_create_ev")
    return h


def host_map_download_evidence(h, first_row=0):
    """The evidence words of rows [first_row, size) as (M - first_row,) uint32; MadIcpError on a map made without the column."""
    m = max(host_map_size(h) - int(first_row), 0)
    out, got = np.empty(max(m, 1), np.uint32), C.c_int64(0)
    _host_map_check(host_lib().madicp_host_map_download_evidence(h, int(first_row), out.ctypes.data_as(_u32p), m, C.byref(got)),
                    "madicp_host_map_download_evidence")
    return out[:got.value].copy()


def host_map_download_min_evidence(h, min_e, with_keys=False, with_attr=False, with_ev=False):
    """madicp_host_map_download_min_evidence: the rows whose evidence word is >= min_e, in row order:
    (rows (n, 3) float32[, keys uint64][, words uint32][, evidence uint32])."""
    m = host_map_size(h)
    xyz, got = np.empty((max(m, 1), 3), np.float32), C.c_int64(0)
    k = np.empty(max(m, 1), np.uint64) if with_keys else None
    w = np.empty(max(m, 1), np.uint32) if with_attr else None
    e = np.empty(max(m, 1), np.uint32) if with_ev else None
    _host_map_check(host_lib().madicp_host_map_download_min_evidence(h, int(min_e), xyz.ctypes.data_as(C.POINTER(C.c_float)),
                                                                     k.ctypes.data_as(_u64p) if with_keys else None,
                                                                     w.ctypes.data_as(_u32p) if with_attr else None,
                                                                     e.ctypes.data_as(_u32p) if with_ev else None, m, C.byref(got)),
                    "madicp_host_map_download_min_evidence")
    g = got.value
    return ((xyz[:g].copy(),) + ((k[:g].copy(),) if with_keys else ()) + ((w[:g].copy(),) if with_attr else ()) +
            ((e[:g].copy(),) if with_ev else ()))


def _evidence_arg(evidence):
    """(hit, miss, cap) or None as the const uint32_t[3] argument of the _create_mom entry points."""
    if evidence is None:
        return None
    hit, miss, cap = evidence
    return (C.c_uint32 * 3)(int(hit), int(miss), int(cap))


def _surfel_buffers(m):
    f = lambda: np.empty((max(m, 1), 3), np.float32)
    return f(), f(), f(), np.empty(max(m, 1), np.uint32)


def host_map_create_mom(voxel, initial_rows, max_rows, max_count, with_attr=False, evidence=None):
    """madicp_host_map_create_mom: a host map with per-voxel moments (the twin of Context.map_create_mom)."""
    h = C.c_void_p()
    _host_map_check(host_lib().madicp_host_map_create_mom(float(voxel), int(initial_rows), int(max_rows), 1 if with_attr else 0,
                                                          _evidence_arg(evidence), int(max_count), C.byref(h)), "madicp_host_map_create_mom")
    return h


def host_map_download_moments(h, first_row=0):
    """The moment words of rows [first_row, size) as (M - first_row, 10) uint64: n, S1[3], S2[6]; MadIcpError without moments."""
    m = max(host_map_size(h) - int(first_row), 0)
    out, got = np.empty((max(m, 1), 10), np.uint64), C.c_int64(0)
    _host_map_check(host_lib().madicp_host_map_download_moments(h, int(first_row), out.ctypes.data_as(_u64p), m, C.byref(got)),
                    "madicp_host_map_download_moments")
    return out[:got.value].copy()


def host_map_download_surfels(h, first_row=0):
    """madicp_host_map_download_surfels: (centroid (M, 3) f32, normal (M, 3) f32, eigenvalues (M, 3) f32, count (M,) u32)."""
    m = max(host_map_size(h) - int(first_row), 0)
    c, nrm, eig, cnt = _surfel_buffers(m)
    got = C.c_int64(0)
    fp = C.POINTER(C.c_float)
    _host_map_check(host_lib().madicp_host_map_download_surfels(h, int(first_row), c.ctypes.data_as(fp), nrm.ctypes.data_as(fp),
                                                                eig.ctypes.data_as(fp), cnt.ctypes.data_as(_u32p), m, C.byref(got)),
                    "madicp_host_map_download_surfels")
    g = got.value
    return c[:g].copy(), nrm[:g].copy(), eig[:g].copy(), cnt[:g].copy()


def host_map_clear(h):
    _host_map_check(host_lib().madicp_host_map_clear(h), "madicp_host_map_clear")


def host_map_destroy(h):
    host_lib().madicp_host_map_destroy(h)


class Context:
    """One device + one stream (include/madicp_hip.h)."""

    def __init__(self, device=0, stream=None):
        h = C.c_void_p()
        _check(hip_lib().madicp_ctx_create(device, C.c_void_p(stream) if stream else None, C.byref(h)))
        self._h = h
        self.device = device

    @classmethod
    def borrowed(cls):
        """The process-wide context the host classes (pymadtree, pymadicp, pypeline.Pipeline) work on —
        madicp_host_device_ctx(), created on first use — wrapped without owning it: close() and __del__ let go of the handle
        and never destroy it.  What sharded.shard_pipeline installs a Pipeline's communicator in."""
        h = host_lib().madicp_host_device_ctx()
        if not h:
            raise MadIcpError("madicp_host_device_ctx: " + hip_lib().madicp_last_error().decode())
        self = cls.__new__(cls)
        self._h = C.c_void_p(h)
        self._borrowed = True
        self.device = int(os.environ.get("MAD_ICP_DEVICE", "0"))
        return self

    def close(self):
        if getattr(self, "_h", None):
            if not getattr(self, "_borrowed", False):
                hip_lib().madicp_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def synchronize(self):
        _check(hip_lib().madicp_ctx_synchronize(self._h))

    def set_option(self, key, value):
        _check(hip_lib().madicp_ctx_set_option(self._h, key.encode(), int(value)))

    def get_option(self, key):
        v = C.c_int64(0)
        _check(hip_lib().madicp_ctx_get_option(self._h, key.encode(), C.byref(v)))
        return v.value

    # ---- trees ----
    def tree_upload(self, nodes, n_leaves):
        nodes = np.ascontiguousarray(nodes, dtype=NODE_DTYPE)
        tid = C.c_int(0)
        _check(hip_lib().madicp_tree_upload(self._h, nodes.ctypes.data_as(C.c_void_p), nodes.shape[0], n_leaves,
                                            C.byref(tid)))
        return tid.value

    def upload(self, host_tree, trusted=False):
        if trusted:
            return self.tree_upload_trusted(host_tree.nodes, host_tree.num_leaves, host_tree.rho2)
        return self.tree_upload(host_tree.nodes, host_tree.num_leaves)

    def tree_upload_trusted(self, nodes, n_leaves, rho2):
        """madicp_tree_upload_trusted: no validation pass (arrays from the product's own builder only)."""
        nodes = np.ascontiguousarray(nodes, dtype=NODE_DTYPE)
        tid = C.c_int(0)
        _check(hip_lib().madicp_tree_upload_trusted(self._h, nodes.ctypes.data_as(C.c_void_p), nodes.shape[0], n_leaves,
                                                    float(rho2), C.byref(tid)))
        return tid.value

    def tree_release(self, tid):
        _check(hip_lib().madicp_tree_release(self._h, tid))

    def tree_download(self, tid, n_nodes):
        out = np.empty(n_nodes, dtype=NODE_DTYPE)
        _check(hip_lib().madicp_tree_download(self._h, tid, out.ctypes.data_as(C.c_void_p), n_nodes))
        return out

    def tree_transform(self, tid, R, t):
        R = _f64(R, (9,))
        t = _f64(t, (3,))
        _check(hip_lib().madicp_tree_transform(self._h, tid, R.ctypes.data_as(_dp), t.ctypes.data_as(_dp)))

    def nn_search(self, tid, queries, want=("leaf", "node", "dist", "depth")):
        q = _f64(queries)
        n = q.shape[0]
        leaf = np.empty(n, np.uint32) if "leaf" in want else None
        node = np.empty(n, np.uint32) if "node" in want else None
        dist = np.empty(n, np.float64) if "dist" in want else None
        depth = np.empty(n, np.int32) if "depth" in want else None
        _check(hip_lib().madicp_nn_search(
            self._h, tid, q.ctypes.data_as(_dp), n,
            leaf.ctypes.data_as(_u32p) if leaf is not None else None,
            node.ctypes.data_as(_u32p) if node is not None else None,
            dist.ctypes.data_as(_dp) if dist is not None else None,
            depth.ctypes.data_as(_i32p) if depth is not None else None))
        return dict(leaf=leaf, node=node, dist=dist, depth=depth)

    def nn_search_device(self, tid, d_queries_ptr, n, d_leaf=None, d_node=None, d_dist=None, d_depth=None):
        _check(hip_lib().madicp_nn_search_device_enqueue(self._h, tid, d_queries_ptr, n, d_leaf, d_node, d_dist,
                                                         d_depth))

    # ---- device front-end: clouds, ingest, deskew, tree build ----
    def cloud_upload(self, xyz):
        a = _f64(xyz)
        cid = C.c_int(0)
        _check(hip_lib().madicp_cloud_upload(self._h, a.ctypes.data_as(_dp), a.shape[0], C.byref(cid)))
        return cid.value

    def cloud_release(self, cid):
        _check(hip_lib().madicp_cloud_release(self._h, cid))

    def cloud_size(self, cid):
        n = C.c_int64(0)
        _check(hip_lib().madicp_cloud_size(self._h, cid, C.byref(n)))
        return n.value

    def cloud_download(self, cid):
        n = self.cloud_size(cid)
        out = np.empty((n, 3))
        _check(hip_lib().madicp_cloud_download(self._h, cid, out.ctypes.data_as(_dp), n))
        return out

    def cloud_ingest_f32(self, records, min_range, max_range, kitti_correction):
        """records: (n, stride >= 3) float32, x y z first (a KITTI .bin is (n,4)).  Returns (cloud id, points kept)."""
        r = np.ascontiguousarray(records, dtype=np.float32)
        if r.ndim != 2 or r.shape[1] < 3:
            raise ValueError("records must be (n, >=3) float32")
        cid, kept = C.c_int(0), C.c_int64(0)
        _check(hip_lib().madicp_cloud_ingest_f32(self._h, r.ctypes.data_as(C.POINTER(C.c_float)), r.shape[0], r.shape[1],
                                                 float(min_range), float(max_range), int(bool(kitti_correction)),
                                                 C.byref(cid), C.byref(kept)))
        return cid.value, kept.value

    def cloud_ingest_records(self, records, min_range, max_range, kitti_correction, layout=None, time_field=None, t_range=None):
        """A driver's byte records (see _records_args) -> a resident, filtered cloud that carries its own normalised stamps.
        Returns (cloud id, points kept, (t0, t1))."""
        r, n, lay, tr = _records_args(records, layout, time_field, t_range)
        cid, kept, rng = C.c_int(0), C.c_int64(0), np.empty(2)
        _check(hip_lib().madicp_cloud_ingest_records(self._h, r.ctypes.data_as(C.c_void_p), n, C.byref(lay), float(min_range),
                                                     float(max_range), int(bool(kitti_correction)),
                                                     tr.ctypes.data_as(_dp) if tr is not None else None, C.byref(cid), C.byref(kept),
                                                     rng.ctypes.data_as(_dp)))
        return cid.value, kept.value, (float(rng[0]), float(rng[1]))

    def cloud_ingest_sources(self, sources, t_range=None):
        """Several sensors' byte records (mad_icp_amd.records.Source objects, see _sources_args) -> ONE resident base-frame cloud
        with one set of stamps on the common clock.  Returns (cloud id, points kept, (t0, t1), survivors per source)."""
        alive, arr, _, _, tr = _sources_args(sources, t_range)
        cid, kept, rng, per = C.c_int(0), C.c_int64(0), np.empty(2), np.zeros(max(len(sources), 1), np.int64)
        _check(hip_lib().madicp_cloud_ingest_sources(self._h, arr, len(sources), tr.ctypes.data_as(_dp) if tr is not None else None,
                                                     C.byref(cid), C.byref(kept), per.ctypes.data_as(_i64p), rng.ctypes.data_as(_dp)))
        return cid.value, kept.value, (float(rng[0]), float(rng[1])), [int(v) for v in per[:len(sources)]]

    def cloud_ingest_sources_attr(self, sources, t_range=None):
        """cloud_ingest_sources for Sources that name an `attribute` (see _attr_fields): the cloud carries the attribute column
        as well.  Returns what cloud_ingest_sources returns."""
        alive, arr, _, _, tr = _sources_args(sources, t_range)
        fields = _attr_fields(sources)
        cid, kept, rng, per = C.c_int(0), C.c_int64(0), np.empty(2), np.zeros(max(len(sources), 1), np.int64)
        _check(hip_lib().madicp_cloud_ingest_sources_attr(self._h, arr, len(sources), fields, tr.ctypes.data_as(_dp) if tr is not None else None,
                                                          C.byref(cid), C.byref(kept), per.ctypes.data_as(_i64p), rng.ctypes.data_as(_dp)))
        return cid.value, kept.value, (float(rng[0]), float(rng[1])), [int(v) for v in per[:len(sources)]]

    def cloud_set_attr(self, cid, attr):
        """Gives a resident cloud an attribute column (one uint32 word per point), or its column new words."""
        w = _u32(attr)
        _check(hip_lib().madicp_cloud_set_attr(self._h, cid, w.ctypes.data_as(_u32p), w.shape[0]))

    def cloud_attr(self, cid):
        """The attribute column a cloud carries, (n,) uint32 in the cloud's order; MadIcpError when it has none."""
        n = self.cloud_size(cid)
        out = np.empty(n, np.uint32)
        _check(hip_lib().madicp_cloud_attr(self._h, cid, out.ctypes.data_as(_u32p), n))
        return out

    def cloud_export_f32_attr(self, cid, R, t, voxel):
        """cloud_export_f32 with the rows' attribute words.  Returns ((M, 3) float32, (M,) uint32)."""
        Rm, tv = _f64(R, (9,)), _f64(t, (3,))
        n = self.cloud_size(cid)
        out, ow, m = np.empty((max(n, 1), 3), np.float32), np.empty(max(n, 1), np.uint32), C.c_int64(0)
        _check(hip_lib().madicp_cloud_export_f32_attr(self._h, cid, Rm.ctypes.data_as(_dp), tv.ctypes.data_as(_dp), float(voxel),
                                                      out.ctypes.data_as(C.POINTER(C.c_float)), ow.ctypes.data_as(_u32p), n, C.byref(m)))
        return out[:m.value].copy(), ow[:m.value].copy()

    def map_create_attr(self, voxel, initial_rows, max_rows):
        """map_create with the attribute column: every row keeps its owning point's word (0 for clouds that carry none)."""
        mid = C.c_int(0)
        _check(hip_lib().madicp_map_create_attr(self._h, float(voxel), int(initial_rows), int(max_rows), C.byref(mid)))
        return mid.value

    def map_download_attr(self, mid, first_row=0):
        """The attribute words of rows [first_row, size) as (M - first_row,) uint32; MadIcpError on a map made without the column."""
        m = max(self.map_size(mid) - int(first_row), 0)
        out, got = np.empty(max(m, 1), np.uint32), C.c_int64(0)
        _check(hip_lib().madicp_map_download_attr(self._h, mid, int(first_row), out.ctypes.data_as(_u32p), m, C.byref(got)))
        return out[:got.value].copy()

    def cloud_stamps(self, cid):
        """The stamps a cloud of cloud_ingest_records carries, (n,) float64 in the cloud's order; MadIcpError when it has none."""
        n = self.cloud_size(cid)
        out = np.empty(n)
        _check(hip_lib().madicp_cloud_stamps(self._h, cid, out.ctypes.data_as(_dp), n))
        return out

    def cloud_export_f32(self, cid, R, t, voxel):
        """A resident cloud out (madicp_cloud_export_f32): through (R (3, 3), t (3,)) as float32 rows, every point in cloud order
        (voxel = 0) or the lowest-index point of every voxel in ascending index order.  Returns (M, 3) float32."""
        Rm, tv = _f64(R, (9,)), _f64(t, (3,))
        n = self.cloud_size(cid)
        out, m = np.empty((max(n, 1), 3), np.float32), C.c_int64(0)
        _check(hip_lib().madicp_cloud_export_f32(self._h, cid, Rm.ctypes.data_as(_dp), tv.ctypes.data_as(_dp), float(voxel),
                                                 out.ctypes.data_as(C.POINTER(C.c_float)), n, C.byref(m)))
        return out[:m.value].copy()

    def map_create(self, voxel, initial_rows, max_rows):
        """A device-resident, append-only voxel map (madicp_map_create): one float32 row per voxel, the first point ever to fall
        into it.  Returns the map id."""
        mid = C.c_int(0)
        _check(hip_lib().madicp_map_create(self._h, float(voxel), int(initial_rows), int(max_rows), C.byref(mid)))
        return mid.value

    def map_insert_cloud(self, mid, cid, R, t):
        """Folds a resident cloud through (R (3, 3), t (3,)) into the map; the cloud is only read.  Returns (rows added, rows the
        map holds)."""
        Rm, tv = _f64(R, (9,)), _f64(t, (3,))
        added, rows = C.c_int64(0), C.c_int64(0)
        _check(hip_lib().madicp_map_insert_cloud(self._h, mid, cid, Rm.ctypes.data_as(_dp), tv.ctypes.data_as(_dp), C.byref(added),
                                                 C.byref(rows)))
        return added.value, rows.value

    def map_size(self, mid):
        rows = C.c_int64(0)
        _check(hip_lib().madicp_map_size(self._h, mid, C.byref(rows)))
        return rows.value

    def map_download_f32(self, mid, first_row=0):
        """Rows [first_row, size) of the map as (M - first_row, 3) float32: what was added since the caller last looked."""
        m = max(self.map_size(mid) - int(first_row), 0)
        out, got = np.empty((max(m, 1), 3), np.float32), C.c_int64(0)
        _check(hip_lib().madicp_map_download_f32(self._h, mid, int(first_row), out.ctypes.data_as(C.POINTER(C.c_float)), m, C.byref(got)))
        return out[:got.value].copy()

    def map_prune(self, mid, center, radius, watermark=0):
        """Removes the rows whose stored float position is farther than radius from center (3,), with their voxels; the kept rows
        close up in order (madicp_map_prune).  Returns (rows removed, rows the map holds, the kept rows among rows [0, watermark)):
        a consumer that had fetched rows [0, watermark) has fetched exactly rows [0, that) of the pruned map."""
        c = _f64(center, (3,))
        removed, rows, mark = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        _check(hip_lib().madicp_map_prune(self._h, mid, c.ctypes.data_as(_dp), float(radius), int(watermark), C.byref(removed),
                                          C.byref(rows), C.byref(mark)))
        return removed.value, rows.value, mark.value

    def map_clear_rays(self, mid, cid, R, t, origin=(0.0, 0.0, 0.0), margin=0.0, watermark=0):
        """Free-space clearing (madicp_map_clear_rays): the rays from origin (3,) to the points of resident cloud cid, taken into
        the map frame by (R (3, 3), t (3,)), are sampled one voxel edge apart, stopping margin short of the point; the rows whose
        voxel a sample falls in and no point of the cloud lies in leave, the kept rows close up in order.  The cloud is only read.
        Returns (rows removed, rows the map holds, the kept rows among rows [0, watermark))."""
        Rm, tv, o = _f64(R, (9,)), _f64(t, (3,)), _f64(origin, (3,))
        removed, rows, mark = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        _check(hip_lib().madicp_map_clear_rays(self._h, mid, cid, Rm.ctypes.data_as(_dp), tv.ctypes.data_as(_dp), o.ctypes.data_as(_dp),
                                               float(margin), int(watermark), C.byref(removed), C.byref(rows), C.byref(mark)))
        return removed.value, rows.value, mark.value

    def map_track_removed(self, mid, on=True):
        """madicp_map_track_removed: from now on the map logs the rows that map_prune and map_clear_rays remove from below their
        watermark (key, float row, word) until map_take_removed fetches them; on=False stops that and frees the log."""
        _check(hip_lib().madicp_map_track_removed(self._h, mid, 1 if on else 0))

    def map_removed_count(self, mid):
        n = C.c_int64(0)
        _check(hip_lib().madicp_map_removed_count(self._h, mid, C.byref(n)))
        return n.value

    def map_take_removed(self, mid, with_attr=False):
        """madicp_map_take_removed: the removal log, oldest first, as (keys (n,) uint64, rows (n, 3) float32[, words (n,) uint32]);
        the log is empty afterwards.  One host synchronisation."""
        n = self.map_removed_count(mid)
        keys, xyz, got = np.empty(max(n, 1), np.uint64), np.empty((max(n, 1), 3), np.float32), C.c_int64(0)
        w = np.empty(max(n, 1), np.uint32) if with_attr else None
        _check(hip_lib().madicp_map_take_removed(self._h, mid, keys.ctypes.data_as(_u64p), xyz.ctypes.data_as(C.POINTER(C.c_float)),
                                                 w.ctypes.data_as(_u32p) if with_attr else None, n, C.byref(got)))
        m = got.value
        return (keys[:m].copy(), xyz[:m].copy()) + ((w[:m].copy(),) if with_attr else ())

    def map_download_keys(self, mid, first_row=0):
        """The stored voxel keys of rows [first_row, size) as (M - first_row,) uint64: a row's identity across prunes."""
        m = max(self.map_size(mid) - int(first_row), 0)
        out, got = np.empty(max(m, 1), np.uint64), C.c_int64(0)
        _check(hip_lib().madicp_map_download_keys(self._h, mid, int(first_row), out.ctypes.data_as(_u64p), m, C.byref(got)))
        return out[:got.value].copy()

    def map_download_rows(self, mid, first_row=0, with_keys=True, with_attr=False):
        """madicp_map_download_rows: the columns of rows [first_row, size) behind ONE host synchronisation:
        (rows (M, 3) float32[, keys (M,) uint64][, words (M,) uint32])."""
        m = max(self.map_size(mid) - int(first_row), 0)
        xyz, got = np.empty((max(m, 1), 3), np.float32), C.c_int64(0)
        k = np.empty(max(m, 1), np.uint64) if with_keys else None
        w = np.empty(max(m, 1), np.uint32) if with_attr else None
        _check(hip_lib().madicp_map_download_rows(self._h, mid, int(first_row), xyz.ctypes.data_as(C.POINTER(C.c_float)),
                                                  k.ctypes.data_as(_u64p) if with_keys else None,
                                                  w.ctypes.data_as(_u32p) if with_attr else None, m, C.byref(got)))
        g = got.value
        return (xyz[:g].copy(),) + ((k[:g].copy(),) if with_keys else ()) + ((w[:g].copy(),) if with_attr else ())

    def map_create_ev(self, voxel, initial_rows, max_rows, hit, miss, cap, with_attr=False):
        """madicp_map_create_ev: a map with the evidence column — a fold gives `hit` to the rows it creates and adds `hit`, once per
        fold and saturating at `cap`, to the older rows it falls into; map_clear_rays takes `miss` from a row it sees through and
        removes it only when that uses the word up.  with_attr: the attribute column as well.  Returns the map id."""
        mid = C.c_int(0)
        _check(hip_lib().madicp_map_create_ev(self._h, float(voxel), int(initial_rows), int(max_rows), 1 if with_attr else 0, int(hit),
                                              int(miss), int(cap), C.byref(mid)))
        return mid.value

    def map_download_evidence(self, mid, first_row=0):
        """The evidence words of rows [first_row, size) as (M - first_row,) uint32; MadIcpError on a map made without the column."""
        m = max(self.map_size(mid) - int(first_row), 0)
        out, got = np.empty(max(m, 1), np.uint32), C.c_int64(0)
        _check(hip_lib().madicp_map_download_evidence(self._h, mid, int(first_row), out.ctypes.data_as(_u32p), m, C.byref(got)))
        return out[:got.value].copy()

    def map_download_min_evidence(self, mid, min_e, with_keys=False, with_attr=False, with_ev=False):
        """madicp_map_download_min_evidence: the rows whose evidence word is >= min_e, in row order, compacted on the device:
        (rows (n, 3) float32[, keys uint64][, words uint32][, evidence uint32])."""
        m = self.map_size(mid)
        xyz, got = np.empty((max(m, 1), 3), np.float32), C.c_int64(0)
        k = np.empty(max(m, 1), np.uint64) if with_keys else None
        w = np.empty(max(m, 1), np.uint32) if with_attr else None
        e = np.empty(max(m, 1), np.uint32) if with_ev else None
        _check(hip_lib().madicp_map_download_min_evidence(self._h, mid, int(min_e), xyz.ctypes.data_as(C.POINTER(C.c_float)),
                                                          k.ctypes.data_as(_u64p) if with_keys else None,
                                                          w.ctypes.data_as(_u32p) if with_attr else None,
                                                          e.ctypes.data_as(_u32p) if with_ev else None, m, C.byref(got)))
        g = got.value
        return ((xyz[:g].copy(),) + ((k[:g].copy(),) if with_keys else ()) + ((w[:g].copy(),) if with_attr else ()) +
                ((e[:g].copy(),) if with_ev else ()))

    def map_create_mom(self, voxel, initial_rows, max_rows, max_count, with_attr=False, evidence=None):
        """madicp_map_create_mom: a map with per-voxel moments — ten 64-bit words per row (n, S1[3], S2[6]) over 16-bit offsets of
        the points that fell into the voxel; a row takes whole folds while its n is below `max_count`.  with_attr / evidence=(hit,
        miss, cap): those columns as well.  Returns the map id."""
        mid = C.c_int(0)
        _check(hip_lib().madicp_map_create_mom(self._h, float(voxel), int(initial_rows), int(max_rows), 1 if with_attr else 0,
                                               _evidence_arg(evidence), int(max_count), C.byref(mid)))
        return mid.value

    def map_download_moments(self, mid, first_row=0):
        """The moment words of rows [first_row, size) as (M - first_row, 10) uint64; MadIcpError on a map made without them."""
        m = max(self.map_size(mid) - int(first_row), 0)
        out, got = np.empty((max(m, 1), 10), np.uint64), C.c_int64(0)
        _check(hip_lib().madicp_map_download_moments(self._h, mid, int(first_row), out.ctypes.data_as(_u64p), m, C.byref(got)))
        return out[:got.value].copy()

    def map_download_surfels(self, mid, first_row=0):
        """madicp_map_download_surfels: (centroid (M, 3) f32, normal (M, 3) f32, eigenvalues (M, 3) f32, count (M,) u32), computed
        on the device from the moments and the stored keys."""
        m = max(self.map_size(mid) - int(first_row), 0)
        c, nrm, eig, cnt = _surfel_buffers(m)
        got = C.c_int64(0)
        fp = C.POINTER(C.c_float)
        _check(hip_lib().madicp_map_download_surfels(self._h, mid, int(first_row), c.ctypes.data_as(fp), nrm.ctypes.data_as(fp),
                                                     eig.ctypes.data_as(fp), cnt.ctypes.data_as(_u32p), m, C.byref(got)))
        g = got.value
        return c[:g].copy(), nrm[:g].copy(), eig[:g].copy(), cnt[:g].copy()

    def map_query(self, mid, cid, R, t, reach=1, max_dist=float("inf"), per_point=True, with_keys=False, with_attr=False, with_ev=False):
        """madicp_map_query_cloud: for every point of resident cloud cid taken through (R (3, 3), t (3,)) the nearest map row of its
        voxel neighbourhood (reach 0: its own voxel, 1: the 27 around it), found where the map lives; the map is only read.
        Returns ((candidates, matched, within max_dist), row (n,) int32, d2 (n,) float64[, keys uint64][, words uint32][, evidence
        uint32]) — row -1, d2 +inf, key all ones, words 0 where there is none — or, with per_point=False (the scoring form: no
        per-point copy), the three counts alone.  One host synchronisation."""
        Rm, tv = _f64(R, (9,)), _f64(t, (3,))
        n = self.cloud_size(cid)
        bufs, args = _query_buffers(n, per_point, with_keys, with_attr, with_ev)
        counts = np.zeros(3, np.uint64)
        _check(hip_lib().madicp_map_query_cloud(self._h, mid, cid, Rm.ctypes.data_as(_dp), tv.ctypes.data_as(_dp), int(reach),
                                                float(max_dist), *args, n, counts.ctypes.data_as(_u64p)))
        return _query_answer(counts, bufs, n, per_point)

    def map_register_cloud(self, mid, cid, R, t, iterations, reach=1, max_dist=float("inf"), rho=float("inf"), min_count=3, flat=1.0,
                           per_point=False):
        """madicp_map_register_cloud: `iterations` rounds of point-to-plane Gauss-Newton of resident cloud cid against the surfels
        of moments map mid, from the pose (R (3, 3), t (3,)), all on the device; the map is only read.  Returns dict(R, t, X, H, b,
        chi2, counts) with one row per linearisation — row k at X[k], the last at the returned pose — and, with per_point (only
        with iterations == 0), row (n,) int32 and e (n,) float64.  One host synchronisation."""
        n = self.cloud_size(cid)

        def call(*args):
            _check(hip_lib().madicp_map_register_cloud(self._h, mid, cid, *args))

        return _align_call(call, n, R, t, iterations, reach, max_dist, rho, min_count, flat, per_point)

    def map_clear(self, mid):
        _check(hip_lib().madicp_map_clear(self._h, mid))

    def map_release(self, mid):
        _check(hip_lib().madicp_map_release(self._h, mid))

    def cloud_deskew_own_stamps(self, cid, velocity, sensor_hz, want_chunks=False):
        """cloud_deskew_stamped from the stamps the cloud carries itself.  Returns the chunks (n,) int32 when asked for."""
        v = _f64(velocity, (6,))
        chunks = np.empty(self.cloud_size(cid), np.int32) if want_chunks else None
        _check(hip_lib().madicp_cloud_deskew_own_stamps(self._h, cid, v.ctypes.data_as(_dp), float(sensor_hz),
                                                        chunks.ctypes.data_as(_i32p) if want_chunks else None))
        return chunks

    def cloud_deskew(self, cid, velocity, sensor_hz, want_chunks=False):
        v = _f64(velocity, (6,))
        chunks = np.empty(self.cloud_size(cid), np.int32) if want_chunks else None
        _check(hip_lib().madicp_cloud_deskew(self._h, cid, v.ctypes.data_as(_dp), float(sensor_hz),
                                             chunks.ctypes.data_as(_i32p) if want_chunks else None))
        return chunks

    def cloud_deskew_stamped(self, cid, stamps, velocity, sensor_hz, want_chunks=False):
        """Motion compensation from per-point timestamps in [0, 1] (one per point, input order kept).  Returns the chunk of
        every point (n,) int32 when asked for, else None."""
        st = np.ascontiguousarray(stamps, dtype=np.float64).reshape(-1)
        v = _f64(velocity, (6,))
        chunks = np.empty(st.shape[0], np.int32) if want_chunks else None
        _check(hip_lib().madicp_cloud_deskew_stamped(self._h, cid, st.ctypes.data_as(_dp), st.shape[0], v.ctypes.data_as(_dp),
                                                     float(sensor_hz), chunks.ctypes.data_as(_i32p) if want_chunks else None))
        return chunks

    def tree_build(self, cid, b_max, b_min):
        """MAD-tree of a resident cloud, built on the device.  Returns (tree id, leaves)."""
        tid, nl = C.c_int(0), C.c_int32(0)
        _check(hip_lib().madicp_tree_build(self._h, cid, float(b_max), float(b_min), C.byref(tid), C.byref(nl)))
        return tid.value, nl.value

    def tree_build_begin(self, xyz, b_max, b_min):
        """Look-ahead: copy the scan and enqueue its construction on the library's build stream; returns at once."""
        a = _f64(xyz)
        _check(hip_lib().madicp_tree_build_begin(self._h, a.ctypes.data_as(_dp), a.shape[0], float(b_max), float(b_min)))

    def tree_build_end(self):
        """... and collect it.  Returns (tree id, leaves)."""
        tid, nl = C.c_int(0), C.c_int32(0)
        _check(hip_lib().madicp_tree_build_end(self._h, C.byref(tid), C.byref(nl)))
        return tid.value, nl.value

    def tree_build_cancel(self):
        _check(hip_lib().madicp_tree_build_cancel(self._h))

    def tree_info(self, tid):
        nn, nl = C.c_int32(0), C.c_int32(0)
        _check(hip_lib().madicp_tree_info(self._h, tid, C.byref(nn), C.byref(nl)))
        return nn.value, nl.value

    def tree_build_stats(self):
        out = np.zeros(130, np.int32)
        _check(hip_lib().madicp_tree_build_stats(self._h, out.ctypes.data_as(_i32p)))
        return dict(max_level=int(out[0]), lane_subtrees=int(out[1]), wave_nodes=out[2:66].copy(), chip_nodes=out[66:130].copy())

    def tree_build_points(self, n):
        """the points of the last synchronous device build in the order the construction left them (diagnostics)"""
        out = np.empty((int(n), 3))
        _check(_aid("madicp_debug_tree_build_points")(self._h, out.ctypes.data_as(_dp), int(n)))
        return out

    def tree_rho(self, tid):
        """the rho the screening test of this tree runs with (diagnostics: the measurement build only)"""
        rho = C.c_double(0.0)
        _check(_aid("madicp_debug_tree_rho")(self._h, int(tid), C.byref(rho)))
        return rho.value

    # ---- moving ----
    def moving_upload(self, leaf_means):
        m = _f64(leaf_means)
        mid = C.c_int(0)
        _check(hip_lib().madicp_moving_upload(self._h, m.ctypes.data_as(_dp), m.shape[0], C.byref(mid)))
        return mid.value

    def moving_update(self, mid, leaf_means):
        m = _f64(leaf_means)
        _check(hip_lib().madicp_moving_update(self._h, mid, m.ctypes.data_as(_dp), m.shape[0]))

    def moving_release(self, mid):
        _check(hip_lib().madicp_moving_release(self._h, mid))

    # ---- registration ----
    @staticmethod
    def _ids(ids):
        arr = (C.c_int * len(ids))(*[int(i) for i in ids])
        return arr

    def icp_linearize(self, mid, tree_ids, T, params, L, want_corr=True):
        K = len(tree_ids)
        X = pose12(T)
        H, b = np.empty((6, 6)), np.empty(6)
        corr = np.empty((K, L), np.uint32) if want_corr else None
        matched = np.empty(L, np.uint8)
        visits = C.c_uint64(0)
        p = IcpParams(*params)
        _check(hip_lib().madicp_icp_linearize(self._h, mid, self._ids(tree_ids), K, X.ctypes.data_as(_dp), C.byref(p),
                                              H.ctypes.data_as(_dp), b.ctypes.data_as(_dp),
                                              corr.ctypes.data_as(_u32p) if want_corr else None,
                                              matched.ctypes.data_as(_u8p), C.byref(visits)))
        return dict(H=H, b=b, corr=corr, matched=matched, visits=visits.value)

    def icp_register(self, mid, tree_ids, T, params, n_iters, L):
        K = len(tree_ids)
        X = pose12(T)
        H, b = np.empty((6, 6)), np.empty(6)
        matched = np.empty(L, np.uint8)
        X_iters = np.empty((n_iters, 12))
        visits = C.c_uint64(0)
        p = IcpParams(*params)
        _check(hip_lib().madicp_icp_register(self._h, mid, self._ids(tree_ids), K, X.ctypes.data_as(_dp), C.byref(p),
                                             n_iters, H.ctypes.data_as(_dp), b.ctypes.data_as(_dp),
                                             matched.ctypes.data_as(_u8p), X_iters.ctypes.data_as(_dp),
                                             C.byref(visits)))
        return dict(T=pose44(X), X=X, H=H, b=b, matched=matched, X_iters=X_iters, visits=visits.value)

    # ---- streamed registrations (new scan in -> X / H / b / flags out) ----
    def stream_submit(self, leaf_means, tree_ids, T, params, n_iters):
        m = _f64(leaf_means)
        X = pose12(T)
        p = IcpParams(*params)
        tk = C.c_int(-1)
        _check(hip_lib().madicp_stream_submit(self._h, m.ctypes.data_as(_dp), m.shape[0], self._ids(tree_ids), len(tree_ids),
                                              X.ctypes.data_as(_dp), C.byref(p), n_iters, C.byref(tk)))
        return tk.value

    def stream_submit_tree(self, moving_tid, tree_ids, T, params, n_iters):
        X = pose12(T)
        p = IcpParams(*params)
        tk = C.c_int(-1)
        _check(hip_lib().madicp_stream_submit_tree(self._h, moving_tid, self._ids(tree_ids), len(tree_ids),
                                                   X.ctypes.data_as(_dp), C.byref(p), n_iters, C.byref(tk)))
        return tk.value

    def stream_collect(self, ticket, L=0):
        X, H, b = np.empty(12), np.empty((6, 6)), np.empty(6)
        matched = np.empty(L, np.uint8) if L else None
        nm = C.c_int32(0)
        visits = C.c_uint64(0)
        _check(hip_lib().madicp_stream_collect(self._h, ticket, X.ctypes.data_as(_dp), H.ctypes.data_as(_dp),
                                               b.ctypes.data_as(_dp), matched.ctypes.data_as(_u8p) if L else None,
                                               C.byref(nm), C.byref(visits)))
        return dict(T=pose44(X), X=X, H=H, b=b, matched=matched, n_matched=nm.value, visits=visits.value)

    # ---- measurement aids ----
    def nn_time_descend(self, tid, queries, reps=20):
        """(avg microseconds per nn_descend launch over the queries, internal nodes visited per launch)."""
        q = _f64(queries)
        us = C.c_double(0.0)
        depth = C.c_uint64(0)
        _check(_aid("madicp_nn_time_descend")(self._h, tid, q.ctypes.data_as(_dp), q.shape[0], reps, C.byref(us),
                                                C.byref(depth)))
        return us.value, depth.value

    def gather16_us(self, region_bytes, n_gathers, seed=1, reps=3):
        """avg microseconds per launch of n_gathers random 16-byte loads over a region (madicp_debug_gather16)."""
        g = C.c_double(0.0)
        _check(_aid("madicp_debug_gather16")(self._h, int(region_bytes), int(n_gathers), int(seed), int(reps), C.byref(g)))
        return g.value

    def stream_copy_gbs(self, nbytes=1 << 30, reps=10):
        g = C.c_double(0.0)
        _check(_aid("madicp_debug_stream_copy")(self._h, nbytes, reps, C.byref(g)))
        return g.value

    def icp_register_batch_enqueue(self, mids, tree_ids, X0, params, n_iters):
        X0 = _f64(X0, (len(mids), 12))
        p = IcpParams(*params)
        _check(hip_lib().madicp_icp_register_batch_enqueue(self._h, len(mids), self._ids(mids), self._ids(tree_ids),
                                                           len(tree_ids), X0.ctypes.data_as(_dp), C.byref(p), n_iters))

    def icp_time_linearize(self, mids, tree_ids, X0, params, n_launches=50):
        """(avg microseconds per first-round icp_round launch, visits per launch per scan) — see madicp_icp_time_linearize."""
        X0 = _f64(X0, (len(mids), 12))
        p = IcpParams(*params)
        us = C.c_double(0.0)
        visits = np.zeros(len(mids), np.uint64)
        _check(_aid("madicp_icp_time_linearize")(self._h, len(mids), self._ids(mids), self._ids(tree_ids), len(tree_ids),
                                                   X0.ctypes.data_as(_dp), C.byref(p), n_launches, C.byref(us),
                                                   visits.ctypes.data_as(_u64p)))
        return us.value, visits

    def icp_time_registration(self, mids, tree_ids, X0, params, n_iters, reps=30):
        """(avg us per icp_round launch over a registration's rounds, us of icp_final, visits per round per scan,
        nodes really walked per round per scan)."""
        X0 = _f64(X0, (len(mids), 12))
        p = IcpParams(*params)
        lin, sol = C.c_double(0.0), C.c_double(0.0)
        visits = np.zeros(len(mids), np.uint64)
        walked = np.zeros(len(mids), np.uint64)
        _check(_aid("madicp_icp_time_registration")(self._h, len(mids), self._ids(mids), self._ids(tree_ids), len(tree_ids),
                                                      X0.ctypes.data_as(_dp), C.byref(p), n_iters, reps, C.byref(lin),
                                                      C.byref(sol), visits.ctypes.data_as(_u64p), walked.ctypes.data_as(_u64p)))
        return lin.value, sol.value, visits, walked

    def icp_fetch(self, n_scans):
        X, H, b = np.empty((n_scans, 12)), np.empty((n_scans, 6, 6)), np.empty((n_scans, 6))
        nm = np.empty(n_scans, np.int32)
        visits = np.empty(n_scans, np.uint64)
        _check(hip_lib().madicp_icp_fetch(self._h, n_scans, X.ctypes.data_as(_dp), H.ctypes.data_as(_dp),
                                          b.ctypes.data_as(_dp), nm.ctypes.data_as(_i32p),
                                          visits.ctypes.data_as(_u64p)))
        return dict(X=X, H=H, b=b, n_matched=nm, visits=visits)

    def moving_update_async(self, mid, leaf_means):
        """madicp_moving_update on the copy stream (beside the batch in flight; ordered by the library)"""
        m = _f64(leaf_means)
        _check(hip_lib().madicp_moving_update_async(self._h, mid, m.ctypes.data_as(_dp), m.shape[0]))

    def icp_publish_enqueue(self, n_scans):
        """ticket for the results of the batch enqueued last (carried to the host by a kernel behind it)"""
        tk = C.c_int(-1)
        _check(hip_lib().madicp_icp_publish_enqueue(self._h, n_scans, C.byref(tk)))
        return tk.value

    def icp_publish_collect(self, ticket, n_scans):
        X, H, b = np.empty((n_scans, 12)), np.empty((n_scans, 6, 6)), np.empty((n_scans, 6))
        nm = np.empty(n_scans, np.int32)
        visits = np.empty(n_scans, np.uint64)
        _check(hip_lib().madicp_icp_publish_collect(self._h, ticket, n_scans, X.ctypes.data_as(_dp), H.ctypes.data_as(_dp),
                                                    b.ctypes.data_as(_dp), nm.ctypes.data_as(_i32p), visits.ctypes.data_as(_u64p)))
        return dict(X=X, H=H, b=b, n_matched=nm, visits=visits)

    def icp_fetch_matched(self, scan, L):
        out = np.empty(L, np.uint8)
        _check(hip_lib().madicp_icp_fetch_matched(self._h, scan, out.ctypes.data_as(_u8p), L))
        return out

    def icp_register_batch(self, mids, tree_ids, X0, params, n_iters):
        self.icp_register_batch_enqueue(mids, tree_ids, X0, params, n_iters)
        return self.icp_fetch(len(mids))

    # ---- multi-GPU ----
    @staticmethod
    def comm_unique_id():
        buf = (C.c_uint8 * 128)()
        _check(hip_lib().madicp_comm_unique_id(buf))
        return bytes(buf)

    def comm_init(self, unique_id, n_ranks, rank):
        buf = (C.c_uint8 * 128)(*unique_id)
        _check(hip_lib().madicp_comm_init(self._h, buf, n_ranks, rank))

    def comm_init_host(self, n_ranks, rank, all_reduce):
        """Host-staged transport (madicp_comm_init_host): `all_reduce(array, kind)` must reduce the numpy array IN PLACE
        over all ranks (kind REDUCE_SUM_F64: float64 sum; REDUCE_MAX_U8: uint8 max).  Exceptions become MADICP_ERR_COMM."""
        def _cb(_user, buf, count, kind):
            try:
                ctype = C.c_double if kind == REDUCE_SUM_F64 else C.c_uint8
                arr = np.ctypeslib.as_array(C.cast(buf, C.POINTER(ctype)), shape=(count,))
                all_reduce(arr, kind)
                return 0
            except Exception as e:  # noqa: BLE001 — must not unwind through the C frame
                self._host_ar_error = e
                return 1

        self._host_ar_cb = HOST_ALLREDUCE_FN(_cb)  # (kept alive as long as the library may call it)
        _check(hip_lib().madicp_comm_init_host(self._h, n_ranks, rank, self._host_ar_cb, None))

    def p2p_export(self):
        """This rank's mailbox as a 64-byte hipIpcMemHandle_t (madicp_p2p_export; allocated on first call)."""
        buf = (C.c_uint8 * 64)()
        _check(hip_lib().madicp_p2p_export(self._h, buf))
        return bytes(buf)

    def p2p_attach(self, handles, n_ranks, rank):
        """Map every rank's mailbox: `handles` = the ranks' 64-byte handles in rank order (madicp_p2p_attach)."""
        blob = b"".join(handles)
        if len(blob) != 64 * n_ranks:
            raise ValueError("expected %d handles of 64 bytes" % n_ranks)
        buf = (C.c_uint8 * len(blob))(*blob)
        _check(hip_lib().madicp_p2p_attach(self._h, buf, n_ranks, rank))

    def p2p_detach(self):
        _check(hip_lib().madicp_p2p_detach(self._h))

    def comm_destroy(self):
        _check(hip_lib().madicp_comm_destroy(self._h))
