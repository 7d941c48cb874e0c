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
_fp = C.POINTER(C.c_float)

# The voxel map's entry points, once for both libraries: (name after madicp_map_, name after madicp_host_map_, the C argument types
# after the handle — (context, map id) on the device, the map on the host).  Three markers stand for what differs between the sides:
_SCAN = "scan"            # the scan: a cloud id on the device, (xyz, n) on the host
_SCAN_ATTR = "scan+attr"  # ... the host's (xyz, attribute words, n); a device cloud carries its words itself
_NEW = "new"              # a create's last argument, the new map: int* id after the context, madicp_host_map** with no handle at all
_SIZING = [C.c_double, C.c_int64, C.c_int64]
_REMOVAL = [C.c_int64, _i64p, _i64p, _i64p]
_WINDOW = [C.c_int64, _i64p]
MAP_ENTRY_POINTS = [
    ("create", "create", _SIZING + [_NEW]),
    ("create_attr", "create_attr", _SIZING + [_NEW]),
    ("create_ev", "create_ev", _SIZING + [C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, _NEW]),
    ("create_mom", "create_mom", _SIZING + [C.c_int, _u32p, C.c_uint32, _NEW]),
    ("insert_cloud", "insert", [_SCAN, _dp, _dp, _i64p, _i64p]),
    ("insert_cloud", "insert_attr", [_SCAN_ATTR, _dp, _dp, _i64p, _i64p]),
    ("size", "size", [_i64p]),
    ("prune", "prune", [_dp, C.c_double] + _REMOVAL),
    ("clear_rays", "clear_rays", [_SCAN, _dp, _dp, _dp, C.c_double] + _REMOVAL),
    ("query_cloud", "query", [_SCAN, _dp, _dp, C.c_int, C.c_double, _i32p, _dp, _u64p, _u32p, _u32p, C.c_int64, _u64p]),
    ("register_cloud", "register", [_SCAN, _dp, _dp, C.POINTER(MapAlignParams), C.c_int, _dp, _dp, _dp, _u64p, _i32p, _dp, C.c_int64]),
    ("score_poses", "score", [_SCAN, _dp, C.c_int64, C.c_int, C.c_double, C.c_int64, _u64p]),
    ("merge_rows", "merge_rows", [C.c_double, _u64p, _fp, _u32p, _u32p, _u64p, C.c_int64, _i64p, _i64p]),
    ("track_removed", "track_removed", [C.c_int]),
    ("removed_count", "removed_count", [_i64p]),
    ("take_removed", "take_removed", [_u64p, _fp, _u32p] + _WINDOW),
    ("download_f32", "download_f32", [C.c_int64, _fp] + _WINDOW),
    ("download_keys", "download_keys", [C.c_int64, _u64p] + _WINDOW),
    ("download_attr", "download_attr", [C.c_int64, _u32p] + _WINDOW),
    ("download_evidence", "download_evidence", [C.c_int64, _u32p] + _WINDOW),
    ("download_moments", "download_moments", [C.c_int64, _u64p] + _WINDOW),
    ("download_rows", "download_rows", [C.c_int64, _fp, _u64p, _u32p] + _WINDOW),
    ("download_min_evidence", "download_min_evidence", [C.c_uint32, _fp, _u64p, _u32p, _u32p] + _WINDOW),
    ("download_surfels", "download_surfels", [C.c_int64, _fp, _fp, _fp, _u32p] + _WINDOW),
    ("clear", "clear", []),
    ("release", "destroy", []),
]


def map_argtypes(device):
    """{entry point: argtypes} of one library's side of MAP_ENTRY_POINTS"""
    scan = {_SCAN: [C.c_int] if device else [_dp, C.c_int64], _SCAN_ATTR: [C.c_int] if device else [_dp, _u32p, C.c_int64],
            _NEW: [_ip] if device else [C.POINTER(C.c_void_p)]}
    out = {}
    for dev_name, host_name, args in MAP_ENTRY_POINTS:
        handle = ([C.c_void_p] if device else []) + ([] if _NEW in args else [C.c_int if device else C.c_void_p])
        out[("madicp_map_" + dev_name) if device else ("madicp_host_map_" + host_name)] = handle + [t for a in args for t in scan.get(a, [a])]
    return out

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
        L.madicp_cloud_export_f32.argtypes = [C.c_void_p, C.c_int, _dp, _dp, C.c_double, C.POINTER(C.c_float), C.c_int64, _i64p]
        for name, argtypes in map_argtypes(device=True).items():
            getattr(L, name).argtypes = argtypes
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
        L.madicp_host_ingest_sources_attr.argtypes = [C.POINTER(RecordSourceC), C.c_int, C.POINTER(AttrFieldC), _dp, _dp, _dp, _u32p, _i64p,
                                                      _i64p, _dp]
        L.madicp_host_cloud_export_f32_attr.argtypes = [_dp, _u32p, C.c_int64, _dp, _dp, C.c_double, C.POINTER(C.c_float), _u32p, C.c_int64,
                                                        _i64p]
        for name, argtypes in map_argtypes(device=False).items():
            getattr(L, name).argtypes = argtypes
        L.madicp_host_map_destroy.restype = None
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


_PTR = {np.float32: _fp, np.float64: _dp, np.int32: _i32p, np.uint32: _u32p, np.uint64: _u64p}


def _ptr(a):
    """an array as the pointer argument of its element type (None: not asked for)"""
    return None if a is None else a.ctypes.data_as(_PTR[a.dtype.type])


# the columns a map hands out: (shape of one row's entry, dtype)
_XYZ, _KEYS, _WORDS, _MOMENTS = ((3,), np.float32), ((), np.uint64), ((), np.uint32), ((10,), np.uint64)


def pose_rows(poses):
    """K poses as the (K, 12) float64 rows the scoring entry points take — R row-major, then t — from (K, 12) or (K, 4, 4)"""
    P = np.asarray(poses, np.float64)
    if P.ndim == 3 and P.shape[1:] == (4, 4):
        P = np.concatenate([P[:, :3, :3].reshape(-1, 9), P[:, :3, 3]], axis=1)
    if P.ndim != 2 or P.shape[1] != 12:
        raise ValueError("poses must be (K, 12) or (K, 4, 4)")
    return np.ascontiguousarray(P)


class _Map:
    """One voxel map, every operation once; Context.map_* (the device's) and host_map_* (the twin's) are these and the
    Context methods document them.  HostMap and DeviceMap say how a call reaches C (create, _call) and what a scan becomes as C
    arguments (_scan): a resident cloud's id on the device, xyz (n, 3) float64 on the host."""
    _NAMES = {}  # the operations whose entry point is named otherwise on this side

    @staticmethod
    def _creation(voxel, initial_rows, max_rows, with_attr=False, evidence=None, max_count=None):
        """(the create entry point of a combination of columns, its arguments before the new map)"""
        sizing = (float(voxel), int(initial_rows), int(max_rows))
        if evidence is not None:
            hit, miss, cap = (int(v) for v in evidence)
        if max_count is not None:
            ev = None if evidence is None else (C.c_uint32 * 3)(hit, miss, cap)
            return "create_mom", sizing + (1 if with_attr else 0, ev, int(max_count))
        if evidence is not None:
            return "create_ev", sizing + (1 if with_attr else 0, hit, miss, cap)
        return ("create_attr" if with_attr else "create"), sizing

    def _fetch(self, op, m, columns, *lead):
        """`op` into one buffer of m rows per column asked for (None: not asked for); the copies of what it wrote"""
        bufs = [None if c is None else np.empty((max(m, 1),) + c[0], c[1]) for c in columns]
        got = C.c_int64(0)
        self._call(op, *lead, *[_ptr(b) for b in bufs], m, C.byref(got))
        return tuple(b[:got.value].copy() for b in bufs if b is not None)

    def _window(self, op, first_row, *columns):
        return self._fetch(op, max(self.size() - int(first_row), 0), columns, int(first_row))

    def _removal(self, op, *args):
        removed, rows, mark = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        self._call(op, *args, C.byref(removed), C.byref(rows), C.byref(mark))
        return removed.value, rows.value, mark.value

    def size(self):
        rows = C.c_int64(0)
        self._call("size", C.byref(rows))
        return rows.value

    def insert(self, scan, R, t, *attr):
        """*attr (the host's insert_attr): the scan's words or None, where it is not a cloud that carries them"""
        Rm, tv = _f64(R, (9,)), _f64(t, (3,))
        added, rows = C.c_int64(0), C.c_int64(0)
        self._call("insert_attr" if attr else "insert", *self._scan(scan, *attr)[0], _ptr(Rm), _ptr(tv), C.byref(added), C.byref(rows))
        return added.value, rows.value

    def prune(self, center, radius, watermark=0):
        return self._removal("prune", _ptr(_f64(center, (3,))), float(radius), int(watermark))

    def clear_rays(self, scan, R, t, origin=(0.0, 0.0, 0.0), margin=0.0, watermark=0):
        Rm, tv, o = _f64(R, (9,)), _f64(t, (3,)), _f64(origin, (3,))
        return self._removal("clear_rays", *self._scan(scan)[0], _ptr(Rm), _ptr(tv), _ptr(o), float(margin), int(watermark))

    def query(self, scan, R, t, reach=1, max_dist=float("inf"), per_point=True, with_keys=False, with_attr=False, with_ev=False):
        Rm, tv = _f64(R, (9,)), _f64(t, (3,))
        where, n = self._scan(scan, sized=True)
        asked = (per_point, per_point, with_keys, with_attr, with_ev)
        bufs = [np.empty(max(n, 1), dt) if a else None for a, dt in zip(asked, (np.int32, np.float64, np.uint64, np.uint32, np.uint32))]
        counts = np.zeros(3, np.uint64)
        self._call("query", *where, _ptr(Rm), _ptr(tv), int(reach), float(max_dist), *[_ptr(b) for b in bufs], n, _ptr(counts))
        c = tuple(int(v) for v in counts)
        return (c,) + tuple(b[:n].copy() for b in bufs if b is not None) if per_point else c

    def register(self, scan, R, t, iterations, reach=1, max_dist=float("inf"), rho=float("inf"), min_count=3, flat=1.0, per_point=False):
        where, n = self._scan(scan, sized=True)
        Rm, tv = _f64(R, (9,)), _f64(t, (3,))
        k1 = max(int(iterations), 0) + 1
        params = MapAlignParams(int(reach), float(max_dist), float(rho), int(min_count), float(flat))
        out_R, out_t = np.zeros(9), np.zeros(3)
        trace, counts = np.zeros((k1, 40)), np.zeros((k1, 4), np.uint64)  # a trace row: X[12] | H[21], the upper triangle | b[6] | chi2
        row = np.empty(max(n, 1), np.int32) if per_point else None
        e = np.empty(max(n, 1), np.float64) if per_point else None
        self._call("register", *where, _ptr(Rm), _ptr(tv), C.byref(params), int(iterations), _ptr(out_R), _ptr(out_t), _ptr(trace),
                   _ptr(counts), _ptr(row), _ptr(e), n)
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

    def score(self, scan, poses, reach=1, max_dist=float("inf"), stride=1):
        P = pose_rows(poses)
        counts = np.zeros((max(P.shape[0], 1), 3), np.uint64)
        self._call("score", *self._scan(scan)[0], _ptr(P), P.shape[0], int(reach), float(max_dist), int(stride), _ptr(counts))
        return counts[:P.shape[0]]

    def merge_rows(self, voxel, keys, rows, words=None, ev=None, mom=None):
        """a batch of saved rows in: keys (n,) uint64, rows (n, 3) float32 and the columns the map has (None: not given) — what
        download_rows / download_evidence / download_moments hand out; bits are passed on as they are (no conversion of values)"""
        k = np.ascontiguousarray(keys, dtype=np.uint64).reshape(-1)
        n = k.shape[0]
        x = np.ascontiguousarray(rows, dtype=np.float32).reshape(-1, 3)
        w, e = (None if a is None else _u32(a) for a in (words, ev))
        M = None if mom is None else np.ascontiguousarray(mom, dtype=np.uint64).reshape(-1, 10)
        if any(a is not None and a.shape[0] != n for a in (x, w, e, M)):
            raise ValueError("one entry of every column per key")
        added, total = C.c_int64(0), C.c_int64(0)
        self._call("merge_rows", float(voxel), _ptr(k), _ptr(x), _ptr(w), _ptr(e), _ptr(M), n, C.byref(added), C.byref(total))
        return added.value, total.value

    def track_removed(self, on=True):
        self._call("track_removed", 1 if on else 0)

    def removed_count(self):
        n = C.c_int64(0)
        self._call("removed_count", C.byref(n))
        return n.value

    def take_removed(self, with_attr=False):
        return self._fetch("take_removed", self.removed_count(), (_KEYS, _XYZ, _WORDS if with_attr else None))

    def download_f32(self, first_row=0):
        return self._window("download_f32", first_row, _XYZ)[0]

    def download_keys(self, first_row=0):
        return self._window("download_keys", first_row, _KEYS)[0]

    def download_attr(self, first_row=0):
        return self._window("download_attr", first_row, _WORDS)[0]

    def download_evidence(self, first_row=0):
        return self._window("download_evidence", first_row, _WORDS)[0]

    def download_moments(self, first_row=0):
        return self._window("download_moments", first_row, _MOMENTS)[0]

    def download_rows(self, first_row=0, with_keys=True, with_attr=False):
        return self._window("download_rows", first_row, _XYZ, _KEYS if with_keys else None, _WORDS if with_attr else None)

    def download_min_evidence(self, min_e, with_keys=False, with_attr=False, with_ev=False):
        columns = (_XYZ, _KEYS if with_keys else None, _WORDS if with_attr else None, _WORDS if with_ev else None)
        return self._fetch("download_min_evidence", self.size(), columns, int(min_e))

    def download_surfels(self, first_row=0):
        return self._window("download_surfels", first_row, _XYZ, _XYZ, _XYZ, _WORDS)

    def clear(self):
        self._call("clear")


class HostMap(_Map):
    """The host twin (madicp_host_map_*, include/madicp_host.h) behind a handle that HostMap.create made; close() frees it."""
    def __init__(self, handle):
        self._h = handle

    @classmethod
    def create(cls, *spec, **more):
        """voxel, initial_rows, max_rows, with_attr=False, evidence=None, max_count=None"""
        op, args = cls._creation(*spec, **more)
        h = C.c_void_p()
        _host_map_check(getattr(host_lib(), "madicp_host_map_" + op)(*args, C.byref(h)), "madicp_host_map_" + op)
        return cls(h)

    def _call(self, op, *args):
        name = "madicp_host_map_" + self._NAMES.get(op, op)
        _host_map_check(getattr(host_lib(), name)(self._h, *args), name)

    def _scan(self, xyz, *attr, sized=False):
        a = _f64(xyz).reshape(-1, 3)
        n = a.shape[0]
        w = None if not attr or attr[0] is None else _u32(attr[0])
        if w is not None and w.shape[0] != n:
            raise ValueError("one attribute word per point")
        return (_ptr(a) if n else None,) + ((_ptr(w),) if attr else ()) + (n,), n

    def close(self):
        host_lib().madicp_host_map_destroy(self._h)


class DeviceMap(_Map):
    """The map where it lives (madicp_map_*, include/madicp_hip.h): map `mid` of Context `ctx`; close() releases it."""
    _NAMES = {"insert": "insert_cloud", "query": "query_cloud", "register": "register_cloud", "score": "score_poses", "close": "release"}
    score_poses = _Map.score  # (the entry point's name on this side: Context.map_score_poses goes through it)

    def __init__(self, ctx, mid):
        self._ctx, self.mid = ctx, mid

    @classmethod
    def create(cls, ctx, *spec, **more):
        """voxel, initial_rows, max_rows, with_attr=False, evidence=None, max_count=None"""
        op, args = cls._creation(*spec, **more)
        mid = C.c_int(0)
        _check(getattr(hip_lib(), "madicp_map_" + op)(ctx._h, *args, C.byref(mid)))
        return cls(ctx, mid.value)

    def _call(self, op, *args):
        _check(getattr(hip_lib(), "madicp_map_" + self._NAMES.get(op, op))(self._ctx._h, self.mid, *args))

    def _scan(self, cid, sized=False):
        return (cid,), (self._ctx.cloud_size(cid) if sized else None)

    def close(self):
        self._call("close")


# the documented names of the host twin: h is what host_map_create* returned; Context.map_* has the words for each
def host_map_create(voxel, initial_rows, max_rows): return HostMap.create(voxel, initial_rows, max_rows)._h
def host_map_create_attr(voxel, initial_rows, max_rows): return HostMap.create(voxel, initial_rows, max_rows, True)._h
def host_map_create_ev(voxel, initial_rows, max_rows, hit, miss, cap, with_attr=False):
    return HostMap.create(voxel, initial_rows, max_rows, with_attr, (hit, miss, cap))._h
def host_map_create_mom(voxel, initial_rows, max_rows, max_count, with_attr=False, evidence=None):
    return HostMap.create(voxel, initial_rows, max_rows, with_attr, evidence, max_count)._h
def host_map_insert(h, xyz, R, t): return HostMap(h).insert(xyz, R, t)
def host_map_insert_attr(h, xyz, attr, R, t): return HostMap(h).insert(xyz, R, t, attr)
def host_map_size(h): return HostMap(h).size()
def host_map_prune(h, center, radius, watermark=0): return HostMap(h).prune(center, radius, watermark)
def host_map_clear_rays(h, xyz, R, t, origin=(0.0, 0.0, 0.0), margin=0.0, watermark=0):
    return HostMap(h).clear_rays(xyz, R, t, origin, margin, watermark)
def host_map_query(h, xyz, R, t, reach=1, max_dist=float("inf"), per_point=True, with_keys=False, with_attr=False, with_ev=False):
    return HostMap(h).query(xyz, R, t, reach, max_dist, per_point, with_keys, with_attr, with_ev)
def host_map_register(h, xyz, R, t, iterations, reach=1, max_dist=float("inf"), rho=float("inf"), min_count=3, flat=1.0, per_point=False):
    return HostMap(h).register(xyz, R, t, iterations, reach, max_dist, rho, min_count, flat, per_point)
def host_map_score(h, xyz, poses, reach=1, max_dist=float("inf"), stride=1): return HostMap(h).score(xyz, poses, reach, max_dist, stride)
def host_map_merge_rows(h, voxel, keys, rows, words=None, ev=None, mom=None): return HostMap(h).merge_rows(voxel, keys, rows, words, ev, mom)
def host_map_track_removed(h, on=True): HostMap(h).track_removed(on)
def host_map_removed_count(h): return HostMap(h).removed_count()
def host_map_take_removed(h, with_attr=False): return HostMap(h).take_removed(with_attr)
def host_map_download_f32(h, first_row=0): return HostMap(h).download_f32(first_row)
def host_map_download_keys(h, first_row=0): return HostMap(h).download_keys(first_row)
def host_map_download_attr(h, first_row=0): return HostMap(h).download_attr(first_row)
def host_map_download_evidence(h, first_row=0): return HostMap(h).download_evidence(first_row)
def host_map_download_moments(h, first_row=0): return HostMap(h).download_moments(first_row)
def host_map_download_rows(h, first_row=0, with_keys=True, with_attr=False): return HostMap(h).download_rows(first_row, with_keys, with_attr)
def host_map_download_min_evidence(h, min_e, with_keys=False, with_attr=False, with_ev=False):
    return HostMap(h).download_min_evidence(min_e, with_keys, with_attr, with_ev)
def host_map_download_surfels(h, first_row=0): return HostMap(h).download_surfels(first_row)
def host_map_clear(h): HostMap(h).clear()
def host_map_destroy(h): HostMap(h).close()


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
        return DeviceMap.create(self, voxel, initial_rows, max_rows, True).mid

    def map_download_attr(self, mid, first_row=0):
        """The attribute words of rows [first_row, size) as (M - first_row,) uint32; MadIcpError on a map made without the column."""
        return DeviceMap(self, mid).download_attr(first_row)

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
        return DeviceMap.create(self, voxel, initial_rows, max_rows).mid

    def map_insert_cloud(self, mid, cid, R, t):
        """Folds a resident cloud through (R (3, 3), t (3,)) into the map; the cloud is only read.  Returns (rows added, rows the
        map holds)."""
        return DeviceMap(self, mid).insert(cid, R, t)

    def map_size(self, mid):
        return DeviceMap(self, mid).size()

    def map_download_f32(self, mid, first_row=0):
        """Rows [first_row, size) of the map as (M - first_row, 3) float32: what was added since the caller last looked."""
        return DeviceMap(self, mid).download_f32(first_row)

    def map_prune(self, mid, center, radius, watermark=0):
        """Removes the rows whose stored float position is farther than radius from center (3,), with their voxels; the kept rows
        close up in order (madicp_map_prune).  Returns (rows removed, rows the map holds, the kept rows among rows [0, watermark)):
        a consumer that had fetched rows [0, watermark) has fetched exactly rows [0, that) of the pruned map."""
        return DeviceMap(self, mid).prune(center, radius, watermark)

    def map_clear_rays(self, mid, cid, R, t, origin=(0.0, 0.0, 0.0), margin=0.0, watermark=0):
        """Free-space clearing (madicp_map_clear_rays): the rays from origin (3,) to the points of resident cloud cid, taken into
        the map frame by (R (3, 3), t (3,)), are sampled one voxel edge apart, stopping margin short of the point; the rows whose
        voxel a sample falls in and no point of the cloud lies in leave, the kept rows close up in order.  The cloud is only read.
        Returns (rows removed, rows the map holds, the kept rows among rows [0, watermark))."""
        return DeviceMap(self, mid).clear_rays(cid, R, t, origin, margin, watermark)

    def map_track_removed(self, mid, on=True):
        """madicp_map_track_removed: from now on the map logs the rows that map_prune and map_clear_rays remove from below their
        watermark (key, float row, word) until map_take_removed fetches them; on=False stops that and frees the log."""
        DeviceMap(self, mid).track_removed(on)

    def map_removed_count(self, mid):
        return DeviceMap(self, mid).removed_count()

    def map_take_removed(self, mid, with_attr=False):
        """madicp_map_take_removed: the removal log, oldest first, as (keys (n,) uint64, rows (n, 3) float32[, words (n,) uint32]);
        the log is empty afterwards.  One host synchronisation."""
        return DeviceMap(self, mid).take_removed(with_attr)

    def map_download_keys(self, mid, first_row=0):
        """The stored voxel keys of rows [first_row, size) as (M - first_row,) uint64: a row's identity across prunes."""
        return DeviceMap(self, mid).download_keys(first_row)

    def map_download_rows(self, mid, first_row=0, with_keys=True, with_attr=False):
        """madicp_map_download_rows: the columns of rows [first_row, size) behind ONE host synchronisation:
        (rows (M, 3) float32[, keys (M,) uint64][, words (M,) uint32])."""
        return DeviceMap(self, mid).download_rows(first_row, with_keys, with_attr)

    def map_create_ev(self, voxel, initial_rows, max_rows, hit, miss, cap, with_attr=False):
        """madicp_map_create_ev: a map with the evidence column — a fold gives `hit` to the rows it creates and adds `hit`, once per
        fold and saturating at `cap`, to the older rows it falls into; map_clear_rays takes `miss` from a row it sees through and
        removes it only when that uses the word up.  with_attr: the attribute column as well.  Returns the map id."""
        return DeviceMap.create(self, voxel, initial_rows, max_rows, with_attr, (hit, miss, cap)).mid

    def map_download_evidence(self, mid, first_row=0):
        """The evidence words of rows [first_row, size) as (M - first_row,) uint32; MadIcpError on a map made without the column."""
        return DeviceMap(self, mid).download_evidence(first_row)

    def map_download_min_evidence(self, mid, min_e, with_keys=False, with_attr=False, with_ev=False):
        """madicp_map_download_min_evidence: the rows whose evidence word is >= min_e, in row order, compacted on the device:
        (rows (n, 3) float32[, keys uint64][, words uint32][, evidence uint32])."""
        return DeviceMap(self, mid).download_min_evidence(min_e, with_keys, with_attr, with_ev)

    def map_create_mom(self, voxel, initial_rows, max_rows, max_count, with_attr=False, evidence=None):
        """madicp_map_create_mom: a map with per-voxel moments — ten 64-bit words per row (n, S1[3], S2[6]) over 16-bit offsets of
        the points that fell into the voxel; a row takes whole folds while its n is below `max_count`.  with_attr / evidence=(hit,
        miss, cap): those columns as well.  Returns the map id."""
        return DeviceMap.create(self, voxel, initial_rows, max_rows, with_attr, evidence, max_count).mid

    def map_download_moments(self, mid, first_row=0):
        """The moment words of rows [first_row, size) as (M - first_row, 10) uint64; MadIcpError on a map made without them."""
        return DeviceMap(self, mid).download_moments(first_row)

    def map_download_surfels(self, mid, first_row=0):
        """madicp_map_download_surfels: (centroid (M, 3) f32, normal (M, 3) f32, eigenvalues (M, 3) f32, count (M,) u32), computed
        on the device from the moments and the stored keys."""
        return DeviceMap(self, mid).download_surfels(first_row)

    def map_query(self, mid, cid, R, t, reach=1, max_dist=float("inf"), per_point=True, with_keys=False, with_attr=False, with_ev=False):
        """madicp_map_query_cloud: for every point of resident cloud cid taken through (R (3, 3), t (3,)) the nearest map row of its
        voxel neighbourhood (reach 0: its own voxel, 1: the 27 around it), found where the map lives; the map is only read.
        Returns ((candidates, matched, within max_dist), row (n,) int32, d2 (n,) float64[, keys uint64][, words uint32][, evidence
        uint32]) — row -1, d2 +inf, key all ones, words 0 where there is none — or, with per_point=False (the scoring form: no
        per-point copy), the three counts alone.  One host synchronisation."""
        return DeviceMap(self, mid).query(cid, R, t, reach, max_dist, per_point, with_keys, with_attr, with_ev)

    def map_register_cloud(self, mid, cid, R, t, iterations, reach=1, max_dist=float("inf"), rho=float("inf"), min_count=3, flat=1.0,
                           per_point=False):
        """madicp_map_register_cloud: `iterations` rounds of point-to-plane Gauss-Newton of resident cloud cid against the surfels
        of moments map mid, from the pose (R (3, 3), t (3,)), all on the device; the map is only read.  Returns dict(R, t, X, H, b,
        chi2, counts) with one row per linearisation — row k at X[k], the last at the returned pose — and, with per_point (only
        with iterations == 0), row (n,) int32 and e (n,) float64.  One host synchronisation."""
        return DeviceMap(self, mid).register(cid, R, t, iterations, reach, max_dist, rho, min_count, flat, per_point)

    def map_score_poses(self, mid, cid, poses, reach=1, max_dist=float("inf"), stride=1):
        """madicp_map_score_poses: map_query's three counts (candidates, matched, within max_dist) of resident cloud cid at each
        of K poses — (K, 12) rows of R row-major then t, or (K, 4, 4) — over the points i with i % stride == 0, in one call:
        one upload of the poses, one launch sequence, ONE host synchronisation whatever n, M and K.  Returns (K, 3) uint64, row k
        what map_query(mid, the subsampled cloud, R_k, t_k, reach, max_dist, per_point=False) returns.  The map is only read."""
        return DeviceMap(self, mid).score_poses(cid, poses, reach, max_dist, stride)

    def map_merge_rows(self, mid, voxel, keys, rows, words=None, ev=None, mom=None):
        """madicp_map_merge_rows: a batch of saved rows merged into the map as ONE fold — keys (n,) uint64, rows (n, 3) float32, and
        words (n,) uint32 / ev (n,) uint32 / mom (n, 10) uint64 exactly where the map has that column (what map_download_rows,
        map_download_evidence and map_download_moments return); voxel must equal the map's.  A key the map lacks becomes a row (the
        lowest index that carries it, bits copied), evidence adds and saturates at cap, moments add under the freeze rule.
        Restoring a saved map is merging into an empty one.  Returns (rows added, rows the map holds).  One host synchronisation."""
        return DeviceMap(self, mid).merge_rows(voxel, keys, rows, words, ev, mom)

    def map_clear(self, mid):
        DeviceMap(self, mid).clear()

    def map_release(self, mid):
        DeviceMap(self, mid).close()

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
