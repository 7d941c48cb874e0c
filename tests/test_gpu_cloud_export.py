"""Context.cloud_export_f32 (madicp_cloud_export_f32: fe::voxel_claim / voxel_mark / the tile scan / voxel_rows) on uploaded
clouds against BOTH the numpy restatement of tests/cloud_export_ref.py and the host twin, bit for bit, over the input sets of the
host test; the sizes cover the wavefront, the workgroup, the 1 024-mark scan tile and many workgroups racing on one table."""
import ctypes as C

import numpy as np
import pytest

import cloud_export_ref as E
from mad_icp_amd import capi

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097, 20000]
VOXELS = [0.0, 1e-3, 0.1, 0.5, 50.0, 1e6]
POSES = {"identity": E.IDENTITY, "random": E.random_pose(11)}
INVALID, CAPACITY = -1, -4

_fp = C.POINTER(C.c_float)
_dp = C.POINTER(C.c_double)


def check(ctx, cid, points, R, t, voxel):
    ref = E.export_f32(points, R, t, voxel)
    got = ctx.cloud_export_f32(cid, R, t, voxel)
    assert got.dtype == np.float32 and got.shape == ref.shape, (got.shape, ref.shape, voxel)
    assert E.same_bits(got, ref), voxel
    assert E.same_bits(got, capi.host_cloud_export_f32(points, R, t, voxel)), voxel
    return got


@pytest.mark.parametrize("n", SIZES)
def test_input_sets_bit_for_bit(ctx, n):
    for name, pts in E.input_sets(n, 100 + n):
        cid = ctx.cloud_upload(pts)
        try:
            for pose in sorted(POSES):
                R, t = POSES[pose]
                for voxel in VOXELS:
                    got = check(ctx, cid, pts, R, t, voxel)
                    if voxel == 0.0:
                        assert got.shape[0] == n, name
        finally:
            ctx.cloud_release(cid)


def test_contention_and_probing(ctx):
    R, t = E.IDENTITY
    # 4 096 points in one cell: every lane on one owner word — one row out, and it is row 0
    pts = E.one_cell(4096, 1)
    cid = ctx.cloud_upload(pts)
    got = check(ctx, cid, pts, R, t, 0.5)
    assert got.shape[0] == 1 and E.same_bits(got, pts[:1].astype(np.float32))
    ctx.cloud_release(cid)
    # two cells alternating
    pts = E.two_cells(4096)
    cid = ctx.cloud_upload(pts)
    got = check(ctx, cid, pts, R, t, 0.5)
    assert E.same_bits(got, pts[:2].astype(np.float32))
    ctx.cloud_release(cid)
    # 20 000 distinct cells: n rows out, the table at its highest load
    pts = E.own_cells(20000)
    cid = ctx.cloud_upload(pts)
    assert check(ctx, cid, pts, R, t, 0.5).shape[0] == 20000
    ctx.cloud_release(cid)
    # a 16-beam x 450 synthetic scan at voxel 0.5, through a pose
    pts = E.synthetic_scan()
    Rr, tr = E.random_pose(5)
    cid = ctx.cloud_upload(pts)
    got = check(ctx, cid, pts, Rr, tr, 0.5)
    assert 100 < got.shape[0] < pts.shape[0]
    ctx.cloud_release(cid)


def test_range_edge_and_nonfinite(ctx):
    R, t = E.IDENTITY
    for voxel in (1e-3, 0.5, 50.0, 1e6):
        pts = E.range_edge(voxel)
        cid = ctx.cloud_upload(pts)
        got = check(ctx, cid, pts, R, t, voxel)
        assert E.same_bits(got, pts[[1, 3, 5, 6, 8]].astype(np.float32))
        ctx.cloud_release(cid)
    pts = np.array([[np.nan, 0.0, 0.0], [0.0, np.inf, 0.0], [1e30, 0.0, 0.0]])
    cid = ctx.cloud_upload(pts)
    assert check(ctx, cid, pts, R, t, 0.0).shape == (3, 3)
    assert check(ctx, cid, pts, R, t, 0.5).shape == (0, 3)  # no candidate: OK with zero rows
    ctx.cloud_release(cid)


def test_repeatable_and_the_cloud_is_untouched(ctx):
    pts = E.gaussian(20000, 77)
    R, t = E.random_pose(3)
    cid = ctx.cloud_upload(pts)
    before = ctx.cloud_download(cid)
    a = ctx.cloud_export_f32(cid, R, t, 0.5)
    b = ctx.cloud_export_f32(cid, R, t, 0.5)
    assert a.tobytes() == b.tobytes() and 1000 < a.shape[0] < 20000
    assert ctx.cloud_export_f32(cid, R, t, 0.0).tobytes() == ctx.cloud_export_f32(cid, R, t, 0.0).tobytes()
    assert ctx.cloud_download(cid).tobytes() == before.tobytes() == np.ascontiguousarray(pts).tobytes()
    ctx.cloud_release(cid)


def test_a_cloud_with_stamps_keeps_them(ctx):
    rng = np.random.default_rng(8)
    n = 3000
    dt = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("t", "<f4")])
    rec = np.zeros(n, dt)
    xyz = (rng.normal(size=(n, 3)) * 10.0).astype(np.float32)
    rec["x"], rec["y"], rec["z"], rec["t"] = xyz[:, 0], xyz[:, 1], xyz[:, 2], rng.uniform(0.0, 0.1, n).astype(np.float32)
    cid, kept, _ = ctx.cloud_ingest_records(rec, 0.7, 120.0, 0)
    assert kept > 2000
    stamps, pts = ctx.cloud_stamps(cid), ctx.cloud_download(cid)
    R, t = E.random_pose(4)
    check(ctx, cid, pts, R, t, 0.3)
    check(ctx, cid, pts, R, t, 0.0)
    assert ctx.cloud_stamps(cid).tobytes() == stamps.tobytes() and ctx.cloud_download(cid).tobytes() == pts.tobytes()
    ctx.cloud_release(cid)


def _raw(ctx, cid, R, t, voxel, out, cap, m):
    f = capi.hip_lib().madicp_cloud_export_f32
    return f(ctx._h, cid, None if R is None else R.ctypes.data_as(_dp), None if t is None else t.ctypes.data_as(_dp), voxel,
             None if out is None else out.ctypes.data_as(_fp), cap, None if m is None else C.byref(m))


def test_refusals(ctx):
    pts = E.gaussian(500, 9)
    R, t = np.eye(3).reshape(9).copy(), np.zeros(3)
    sentinel = np.float32(-77.5)
    out = np.full((500, 3), sentinel, np.float32)
    m = C.c_int64(-7)
    cid = ctx.cloud_upload(pts)
    assert _raw(ctx, cid, None, t, 0.5, out, 500, m) == INVALID
    assert _raw(ctx, cid, R, None, 0.5, out, 500, m) == INVALID
    assert _raw(ctx, cid, R, t, 0.5, None, 500, m) == INVALID
    assert _raw(ctx, cid, R, t, 0.5, out, 500, None) == INVALID
    assert _raw(ctx, cid + 1000, R, t, 0.5, out, 500, m) == INVALID
    assert capi.hip_lib().madicp_cloud_export_f32(None, cid, R.ctypes.data_as(_dp), t.ctypes.data_as(_dp), 0.5, out.ctypes.data_as(_fp), 500,
                                                  C.byref(m)) == INVALID
    for bad in (np.nan, np.inf, -np.inf):
        Rb, tb = R.copy(), t.copy()
        Rb[7] = bad
        tb[0] = bad
        assert _raw(ctx, cid, Rb, t, 0.5, out, 500, m) == INVALID
        assert _raw(ctx, cid, R, tb, 0.5, out, 500, m) == INVALID
        assert _raw(ctx, cid, R, t, bad, out, 500, m) == INVALID
    assert _raw(ctx, cid, R, t, -0.5, out, 500, m) == INVALID
    assert m.value == -7 and (out == sentinel).all()
    # capacity: the number needed comes back, nothing is written
    need = E.export_f32(pts, np.eye(3), t, 0.5).shape[0]
    assert 1 < need <= 500
    assert _raw(ctx, cid, R, t, 0.5, out, need - 1, m) == CAPACITY and m.value == need and (out == sentinel).all()
    m.value = -7
    assert _raw(ctx, cid, R, t, 0.0, out, 499, m) == CAPACITY and m.value == 500 and (out == sentinel).all()
    assert _raw(ctx, cid, R, t, 0.5, out, need, m) == 0 and m.value == need  # exactly enough is enough
    assert (out[need:] == sentinel).all() and E.same_bits(out[:need], E.export_f32(pts, np.eye(3), t, 0.5))
    # while a look-ahead build is in flight the scratch is not this call's
    out[:] = sentinel
    m.value = -7
    ctx.tree_build_begin(E.gaussian(3000, 10), 0.2, 0.1)
    try:
        assert _raw(ctx, cid, R, t, 0.5, out, 500, m) == CAPACITY and m.value == -7 and (out == sentinel).all()
    finally:
        tid, _ = ctx.tree_build_end()
        ctx.tree_release(tid)
    assert _raw(ctx, cid, R, t, 0.5, out, 500, m) == 0 and m.value == need
    ctx.cloud_release(cid)


def test_full_size_count(ctx):
    """120 000 points: the count only, against the host twin"""
    rng = np.random.default_rng(120)
    d = rng.normal(size=(120000, 3))
    pts = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(2.0, 60.0, size=(120000, 1))
    R, t = E.random_pose(6)
    cid = ctx.cloud_upload(pts)
    for voxel in (0.2, 0.5):
        assert ctx.cloud_export_f32(cid, R, t, voxel).shape[0] == capi.host_cloud_export_f32(pts, R, t, voxel).shape[0]
    ctx.cloud_release(cid)
