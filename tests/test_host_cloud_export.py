"""The host twin of the export (madicp_host_cloud_export_f32, csrc/host/cloud_export.h) against the numpy restatement of
tests/cloud_export_ref.py, bit for bit (compared as uint32), and every refusal with the output buffer unwritten.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import cloud_export_ref as E
from mad_icp_amd import capi

SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 5000]
VOXELS = [0.0, 1e-3, 0.1, 0.5, 50.0, 1e6]
POSES = {"identity": E.IDENTITY, "random": E.random_pose(11)}

FOLD_SIZES = [1, 63, 64, 65, 257, 1025, 4097]
FOLD_VOXELS = [1e-3, 0.1, 0.5, 50.0, 1e6]

_fp = C.POINTER(C.c_float)
_dp = C.POINTER(C.c_double)


def check(points, R, t, voxel):
    ref = E.export_f32(points, R, t, voxel)
    got = capi.host_cloud_export_f32(points, R, t, voxel)
    assert got.dtype == np.float32 and got.shape == ref.shape, (got.shape, ref.shape)
    assert E.same_bits(got, ref)
    return got


@pytest.mark.parametrize("pose", sorted(POSES))
@pytest.mark.parametrize("n", SIZES)
def test_input_sets_bit_for_bit(natives, n, pose):
    R, t = POSES[pose]
    for name, pts in E.input_sets(n, 100 + n):
        for voxel in VOXELS:
            got = check(pts, R, t, voxel)
            if voxel == 0.0:
                assert got.shape[0] == n, name  # nothing dropped, NaN rows included
            if name == "nonfinite" and voxel > 0.0:
                assert np.isfinite(got).all()  # NaN / inf rows are dropped


def test_cells_on_faces_and_signed_zero(natives):
    R, t = E.IDENTITY
    # -0.25 lies in cell -1, -0.0 and 0.25 in cell 0, 0.5 in cell 1, -0.5 in cell -1, -0.75 in cell -2 (voxel 0.5)
    pts = np.array([[0.25, 0, 0], [-0.0, 0, 0], [-0.25, 0, 0], [-0.5, 0, 0], [0.5, 0, 0], [-0.75, 0, 0], [0.75, 0, 0]], dtype=np.float64)
    got = check(pts, R, t, 0.5)
    assert got[:, 0].tolist() == [0.25, -0.25, 0.5, -0.75]
    # multiples of 0.5 at voxel 0.5, negative ones included: one row per distinct coordinate triple
    faces = E.on_faces(2000, 5)
    faces[faces == -0.25] = 0.0
    got = check(faces, R, t, 0.5)
    assert got.shape[0] == np.unique(faces + 0.0, axis=0).shape[0]


def test_duplicates_one_cell_own_cells(natives):
    R, t = E.IDENTITY
    n = 777
    assert check(E.one_cell(n, 1), R, t, 0.001).shape[0] == 1
    got = check(E.one_cell(n, 1), R, t, 0.5)
    assert E.same_bits(got, E.one_cell(n, 1)[:1].astype(np.float32))  # ... and it is row 0
    assert check(E.own_cells(n), R, t, 0.5).shape[0] == n
    assert check(E.own_cells(n), R, t, 1.0).shape[0] == n
    dup = E.duplicates(n, 2)
    assert check(dup, R, t, 1e-3).shape[0] == np.unique(dup, axis=0).shape[0]
    assert check(E.two_cells(n), R, t, 0.5).shape[0] == 2


def test_nonfinite_rows_pass_at_voxel_zero_only(natives):
    R, t = E.IDENTITY
    pts = np.array([[1.0, 2.0, 3.0], [np.nan, 0.0, 0.0], [0.0, np.inf, 0.0], [0.0, 0.0, -np.inf], [4.0, 5.0, 6.0]])
    got = check(pts, R, t, 0.0)
    assert got.shape[0] == 5 and np.isnan(got[1]).all()  # (0 * inf: the whole row is NaN under the identity too)
    got = check(pts, R, t, 0.5)
    assert got.tolist() == [[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]]
    assert check(pts[1:4], R, t, 0.5).shape == (0, 3)  # no candidate at all: OK with zero rows
    # overflow to +-inf in the OUTPUT is left as IEEE gives it (voxel 0); the cells of such a point are out of range otherwise
    big = np.array([[1e300, -1e300, 1e39]])
    assert check(big, R, t, 0.0).tolist() == [[np.inf, -np.inf, np.inf]]
    assert check(big, R, t, 1e6).shape == (0, 3)


@pytest.mark.parametrize("voxel", [1e-3, 0.5, 50.0, 1e6])
def test_range_edge(natives, voxel):
    R, t = E.IDENTITY
    pts = E.range_edge(voxel)
    got = check(pts, R, t, voxel)
    # q = 2^20 * voxel: cell 2^20, dropped (rows 0, 2, 4); q = -2^20 * voxel: cell -2^20, kept (rows 1, 3, 5); the last double below
    # the upper edge is kept (row 6), the first one beyond the lower edge dropped (row 7); the centre (row 8)
    assert E.same_bits(got, pts[[1, 3, 5, 6, 8]].astype(np.float32))


def _raw(xyz, n, R, t, voxel, out, cap, m):
    f = capi.host_lib().madicp_host_cloud_export_f32
    return f(None if xyz is None else xyz.ctypes.data_as(_dp), n, None if R is None else R.ctypes.data_as(_dp),
             None if t is None else t.ctypes.data_as(_dp), voxel, None if out is None else out.ctypes.data_as(_fp), cap,
             None if m is None else C.byref(m))


def test_refusals_leave_the_output_alone(natives):
    pts = E.gaussian(100, 9)
    R, t = np.eye(3).reshape(9).copy(), np.zeros(3)
    sentinel = np.float32(-77.5)
    out = np.full((100, 3), sentinel, np.float32)
    m = C.c_int64(-7)
    INVALID, CAPACITY = -1, -4
    assert _raw(None, 100, R, t, 0.5, out, 100, m) == INVALID
    assert _raw(pts, 100, None, t, 0.5, out, 100, m) == INVALID
    assert _raw(pts, 100, R, None, 0.5, out, 100, m) == INVALID
    assert _raw(pts, 100, R, t, 0.5, None, 100, m) == INVALID
    assert _raw(pts, 100, R, t, 0.5, out, 100, None) == INVALID
    assert _raw(pts, -1, R, t, 0.5, out, 100, m) == INVALID
    for bad in (np.nan, np.inf, -np.inf):
        Rb, tb = R.copy(), t.copy()
        Rb[4] = bad
        tb[2] = bad
        assert _raw(pts, 100, Rb, t, 0.5, out, 100, m) == INVALID
        assert _raw(pts, 100, R, tb, 0.5, out, 100, m) == INVALID
        assert _raw(pts, 100, R, t, bad, out, 100, m) == INVALID
    assert _raw(pts, 100, R, t, -0.5, out, 100, m) == INVALID
    assert _raw(pts, 100, R, t, -1e-300, out, 100, m) == INVALID
    assert m.value == -7 and (out == sentinel).all()
    # capacity: the number needed comes back, nothing is written
    need = E.export_f32(pts, np.eye(3), t, 0.5).shape[0]
    assert 1 < need <= 100
    assert _raw(pts, 100, R, t, 0.5, out, need - 1, m) == CAPACITY and m.value == need and (out == sentinel).all()
    m.value = -7
    assert _raw(pts, 100, R, t, 0.0, out, 99, m) == CAPACITY and m.value == 100 and (out == sentinel).all()
    # exactly enough is enough, and only those rows are written
    assert _raw(pts, 100, R, t, 0.5, out, need, m) == 0 and m.value == need
    assert (out[need:] == sentinel).all() and E.same_bits(out[:need], E.export_f32(pts, np.eye(3), t, 0.5))
    # an empty cloud and a cloud without a candidate are OK with zero rows
    assert _raw(pts, 0, R, t, 0.5, out, 0, m) == 0 and m.value == 0
    far = np.full((3, 3), 1e30)
    assert _raw(far, 3, R, t, 0.5, out, 0, m) == 0 and m.value == 0


def first_fold(points, R, t, voxel):
    """a fresh host map's first fold of the cloud, downloaded"""
    h = capi.host_map_create(voxel, max(points.shape[0], 1), 1 << 24)
    try:
        capi.host_map_insert(h, points, R, t)
        return capi.host_map_download_f32(h)
    finally:
        capi.host_map_destroy(h)


@pytest.mark.parametrize("n", FOLD_SIZES)
def test_thinned_export_is_a_first_fold(natives, n):
    """voxel > 0: the bytes of a fresh map's first fold of the same cloud, downloaded"""
    for name, pts in E.input_sets(n, 100 + n):
        for pose in sorted(POSES):
            R, t = POSES[pose]
            for voxel in FOLD_VOXELS:
                got = capi.host_cloud_export_f32(pts, R, t, voxel)
                assert got.tobytes() == first_fold(pts, R, t, voxel).tobytes(), (name, pose, voxel)


def test_first_fold_capacity_leaves_the_output_alone(natives):
    pts = E.gaussian(1025, 9)
    R, t = E.random_pose(11)
    need = first_fold(pts, R, t, 0.5).shape[0]
    assert 1 < need < 1025
    sentinel = np.float32(-77.5)
    out = np.full((1025, 3), sentinel, np.float32)
    m = C.c_int64(-7)
    Rf = np.ascontiguousarray(R, dtype=np.float64).reshape(9)
    assert _raw(pts, 1025, Rf, t, 0.5, out, need - 1, m) == -4 and m.value == need and (out == sentinel).all()
