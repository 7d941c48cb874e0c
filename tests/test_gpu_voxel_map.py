"""Context.map_* (madicp_map_*: fe::voxel_claim / voxel_mark / the tile scan / voxel_rows / map_rehash) on uploaded clouds against BOTH
the numpy restatement of tests/voxel_map_ref.py and the host twin, bit for bit after every fold, over the sequences of the host
test; the sizes cover the wavefront, the workgroup, the 1 024-mark scan tile and many workgroups racing on one persistent table."""
import ctypes as C

import numpy as np
import pytest

import cloud_export_ref as E
import voxel_map_ref as V
from mad_icp_amd import capi

pytestmark = pytest.mark.gpu

INVALID, CAPACITY = -1, -4
_fp = C.POINTER(C.c_float)
_dp = C.POINTER(C.c_double)
_i64 = C.POINTER(C.c_int64)


@pytest.fixture
def maps(ctx):
    """map_create whose maps (and the clouds uploaded through `fold`) are released at the end of the test"""
    made = []

    def make(voxel=V.VOXEL, initial_rows=64, max_rows=1 << 24):
        made.append(ctx.map_create(voxel, initial_rows, max_rows))
        return made[-1]

    yield make
    for mid in made:
        ctx.map_release(mid)


def fold(ctx, mid, pts, R, t):
    cid = ctx.cloud_upload(pts)
    try:
        return ctx.map_insert_cloud(mid, cid, R, t)
    finally:
        ctx.cloud_release(cid)


@pytest.mark.parametrize("kind", ["identity", "random"])
@pytest.mark.parametrize("n", V.SIZES)
def test_sequences_bit_for_bit(ctx, maps, n, kind):
    mid = maps()
    twin = capi.host_map_create(V.VOXEL, 64, 1 << 24)
    try:
        prev = np.empty((0, 3), np.float32)
        for pts, R, t, added, want in V.reference(n, kind):
            assert fold(ctx, mid, pts, R, t) == (added, want.shape[0]) == capi.host_map_insert(twin, pts, R, t)
            assert ctx.map_size(mid) == want.shape[0]
            got = ctx.map_download_f32(mid)
            assert got.dtype == np.float32 and E.same_bits(got, want)
            assert got.tobytes() == capi.host_map_download_f32(twin).tobytes()
            assert got[:prev.shape[0]].tobytes() == prev.tobytes()  # prefix stability: a fold changes no row
            assert ctx.map_download_f32(mid, prev.shape[0]).tobytes() == got[prev.shape[0]:].tobytes()  # the window of this fold
            prev = got
        assert prev.shape[0] > 0
    finally:
        capi.host_map_destroy(twin)


def test_contention_and_highest_load(ctx, maps):
    R, t = E.IDENTITY
    # 4 096 points in one cell: every lane on one owner word — one row, and it is row 0; the next frames' points find it settled
    mid = maps()
    pts = E.one_cell(4096, 1)
    assert fold(ctx, mid, pts, R, t) == (1, 1)
    assert E.same_bits(ctx.map_download_f32(mid), pts[:1].astype(np.float32))
    assert fold(ctx, mid, E.one_cell(4096, 2), R, t) == (0, 1) and fold(ctx, mid, pts, R, t) == (0, 1)
    assert E.same_bits(ctx.map_download_f32(mid), pts[:1].astype(np.float32))
    # two cells alternating, then the same cloud again
    mid = maps()
    pts = E.two_cells(4096)
    assert fold(ctx, mid, pts, R, t) == (2, 2) and fold(ctx, mid, pts, R, t) == (0, 2)
    assert E.same_bits(ctx.map_download_f32(mid), pts[:2].astype(np.float32))
    # 20 000 distinct cells into max_rows = 20 000: fits exactly, the table at its highest load (half full)
    n = 20000
    mid = maps(initial_rows=n, max_rows=n)
    pts = E.own_cells(n)
    assert fold(ctx, mid, pts, R, t) == (n, n)
    assert E.same_bits(ctx.map_download_f32(mid), pts.astype(np.float32))


def test_growth_does_not_show(ctx, maps):
    """initial_rows = 1 over six folds of 4 097 points: the block grows (and the table is rehashed) several times; byte-equal to a map
    created large enough never to grow"""
    small, large = maps(initial_rows=1), maps(initial_rows=1 << 16)
    ref = V.RefMap(V.VOXEL)
    for f in range(6):
        pts = E.gaussian(4097, 300 + f, scale=6.0 + f)
        R, t = E.random_pose(60 + f)
        added = ref.insert(pts, R, t)
        assert fold(ctx, small, pts, R, t) == fold(ctx, large, pts, R, t) == (added, ref.size)
        assert ctx.map_download_f32(small).tobytes() == ctx.map_download_f32(large).tobytes()
    assert ref.size > 2 * 4097 and E.same_bits(ctx.map_download_f32(small), ref.rows())


def test_two_maps_interleaved_and_clear(ctx, maps):
    a, b, alone = maps(), maps(voxel=0.25), maps()
    seq_a, seq_b = V.reference(1025, "random"), V.reference(1023, "identity")
    ref_b = V.RefMap(0.25)
    for k in range(max(len(seq_a), len(seq_b))):
        if k < len(seq_a):
            pts, R, t, added, want = seq_a[k]
            assert fold(ctx, a, pts, R, t) == (added, want.shape[0])
        if k < len(seq_b):
            pts, R, t, _, _ = seq_b[k]
            added = ref_b.insert(pts, R, t)
            assert fold(ctx, b, pts, R, t) == (added, ref_b.size)
    for pts, R, t, _, _ in seq_a:
        fold(ctx, alone, pts, R, t)
    first = ctx.map_download_f32(a)
    assert first.tobytes() == ctx.map_download_f32(alone).tobytes() and E.same_bits(first, seq_a[-1][4])
    assert E.same_bits(ctx.map_download_f32(b), ref_b.rows())
    # clear, then the same sequence: the same bytes; the other map is untouched
    ctx.map_clear(a)
    assert ctx.map_size(a) == 0 and ctx.map_download_f32(a).shape == (0, 3)
    for pts, R, t, added, want in seq_a:
        assert fold(ctx, a, pts, R, t) == (added, want.shape[0])
    assert ctx.map_download_f32(a).tobytes() == first.tobytes()
    assert E.same_bits(ctx.map_download_f32(b), ref_b.rows())


@pytest.mark.parametrize("voxel", [1e-3, 0.5, 50.0, 1e6])
def test_range_edge(ctx, maps, voxel):
    R, t = E.IDENTITY
    mid = maps(voxel=voxel)
    pts = E.range_edge(voxel)
    assert fold(ctx, mid, pts, R, t) == (5, 5)
    assert E.same_bits(ctx.map_download_f32(mid), pts[[1, 3, 5, 6, 8]].astype(np.float32))


def test_nonfinite_and_the_fp64_key(ctx, maps):
    R, t = E.IDENTITY
    mid = maps()
    pts = np.array([[np.nan, 0.0, 0.0], [0.0, np.inf, 0.0], [1e30, 0.0, 0.0]])
    assert fold(ctx, mid, pts, R, t) == (0, 0)  # no candidate: OK with zero rows
    ref = V.RefMap(V.VOXEL)
    noisy = E.with_nonfinite(E.gaussian(3000, 3), 4)
    assert fold(ctx, mid, noisy, R, t) == (ref.insert(noisy, R, t), ref.size)
    got = ctx.map_download_f32(mid)
    assert E.same_bits(got, ref.rows()) and np.isfinite(got).all()
    # nextafter(0.5, 0) is stored as float 0.5 in cell 0; 0.5 exactly is cell 1 and must be added: two rows whose floats are equal
    mid = maps(voxel=0.5)
    below, exact = np.array([[np.nextafter(0.5, 0.0), 0.25, 0.25]]), np.array([[0.5, 0.25, 0.25]])
    assert fold(ctx, mid, below, R, t) == (1, 1) and fold(ctx, mid, exact, R, t) == (1, 2) and fold(ctx, mid, below, R, t) == (0, 2)
    got = ctx.map_download_f32(mid)
    assert got[0].tobytes() == got[1].tobytes() and got[0, 0] == np.float32(0.5)


def test_the_cloud_and_its_stamps_are_untouched(ctx, maps):
    rng = np.random.default_rng(8)
    n = 3000
    dt = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("t", "<f4")])
    rec = np.zeros(n, dt)
    xyz = (rng.normal(size=(n, 3)) * 10.0).astype(np.float32)
    rec["x"], rec["y"], rec["z"], rec["t"] = xyz[:, 0], xyz[:, 1], xyz[:, 2], rng.uniform(0.0, 0.1, n).astype(np.float32)
    cid, kept, _ = ctx.cloud_ingest_records(rec, 0.7, 120.0, 0)
    assert kept > 2000
    stamps, pts = ctx.cloud_stamps(cid), ctx.cloud_download(cid)
    mid = maps(voxel=0.3)
    ref = V.RefMap(0.3)
    for seed in (4, 5):
        R, t = E.random_pose(seed)
        assert ctx.map_insert_cloud(mid, cid, R, t) == (ref.insert(pts, R, t), ref.size)
    assert E.same_bits(ctx.map_download_f32(mid), ref.rows())
    assert ctx.cloud_stamps(cid).tobytes() == stamps.tobytes() and ctx.cloud_download(cid).tobytes() == pts.tobytes()
    ctx.cloud_release(cid)


def _insert(ctx, mid, cid, R, t, a, r):
    return capi.hip_lib().madicp_map_insert_cloud(ctx._h, mid, cid, None if R is None else R.ctypes.data_as(_dp),
                                                  None if t is None else t.ctypes.data_as(_dp), None if a is None else C.byref(a),
                                                  None if r is None else C.byref(r))


def test_refusals(ctx, maps):
    L = capi.hip_lib()
    new = C.c_int(-7)
    for voxel, initial, max_rows in ((0.0, 1, 10), (-0.5, 1, 10), (np.nan, 1, 10), (np.inf, 1, 10), (0.5, 0, 10), (0.5, 1, 0),
                                     (0.5, 1, (1 << 30) + 1)):
        assert L.madicp_map_create(ctx._h, voxel, initial, max_rows, C.byref(new)) == INVALID and new.value == -7
    assert L.madicp_map_create(ctx._h, 0.5, 1, 10, None) == INVALID and L.madicp_map_create(None, 0.5, 1, 10, C.byref(new)) == INVALID
    pts = E.gaussian(500, 9)
    R, t = np.eye(3).reshape(9).copy(), np.zeros(3)
    mid = maps(initial_rows=4, max_rows=600)
    cid = ctx.cloud_upload(pts)
    added, rows = ctx.map_insert_cloud(mid, cid, R, t)
    assert 1 < rows == added <= 500
    before = ctx.map_download_f32(mid).tobytes()
    a, r = C.c_int64(-7), C.c_int64(-7)
    assert _insert(ctx, mid, cid, None, t, a, r) == INVALID
    assert _insert(ctx, mid, cid, R, None, a, r) == INVALID
    assert _insert(ctx, mid, cid, R, t, None, r) == INVALID
    assert _insert(ctx, mid, cid, R, t, a, None) == INVALID
    assert _insert(ctx, mid + 1000, cid, R, t, a, r) == INVALID
    assert _insert(ctx, mid, cid + 1000, R, t, a, r) == INVALID
    assert _insert(ctx, cid, cid, R, t, a, r) == INVALID  # a cloud's id is no map's
    assert L.madicp_map_insert_cloud(None, mid, cid, R.ctypes.data_as(_dp), t.ctypes.data_as(_dp), C.byref(a), C.byref(r)) == INVALID
    for bad in (np.nan, np.inf, -np.inf):
        Rb, tb = R.copy(), t.copy()
        Rb[7] = bad
        tb[0] = bad
        assert _insert(ctx, mid, cid, Rb, t, a, r) == INVALID
        assert _insert(ctx, mid, cid, R, tb, a, r) == INVALID
    # max_rows: rows + n > max_rows is refused before any launch, even where no point would be new
    assert rows + 500 > 600 and _insert(ctx, mid, cid, R, t, a, r) == CAPACITY
    assert (a.value, r.value) == (-7, -7) and ctx.map_size(mid) == rows and ctx.map_download_f32(mid).tobytes() == before
    # download: too little room — the number needed, nothing written; a first_row beyond the map; nulls; unknown ids
    sentinel = np.float32(-77.5)
    out = np.full((rows, 3), sentinel, np.float32)
    k = C.c_int64(-7)
    f, o = L.madicp_map_download_f32, out.ctypes.data_as(_fp)
    assert f(ctx._h, mid, 0, o, rows - 1, C.byref(k)) == CAPACITY and k.value == rows and (out == sentinel).all()
    k.value = -7
    assert f(ctx._h, mid, rows + 1, o, rows, C.byref(k)) == INVALID and f(ctx._h, mid, -1, o, rows, C.byref(k)) == INVALID
    assert f(ctx._h, mid, 0, None, rows, C.byref(k)) == INVALID and f(ctx._h, mid, 0, o, rows, None) == INVALID
    assert f(ctx._h, mid + 1000, 0, o, rows, C.byref(k)) == INVALID and f(None, mid, 0, o, rows, C.byref(k)) == INVALID
    assert k.value == -7 and (out == sentinel).all()
    assert f(ctx._h, mid, 3, o, rows - 3, C.byref(k)) == 0 and k.value == rows - 3  # exactly enough is enough
    assert out[:rows - 3].tobytes() == before[36:] and (out[rows - 3:] == sentinel).all()
    assert L.madicp_map_size(ctx._h, mid + 1000, C.byref(k)) == INVALID and L.madicp_map_size(ctx._h, mid, None) == INVALID
    assert L.madicp_map_clear(ctx._h, mid + 1000) == INVALID and L.madicp_map_release(ctx._h, mid + 1000) == INVALID
    # while a look-ahead build is in flight the scratch is not this call's: refused, map unchanged; the same fold succeeds afterwards
    room = maps()
    ctx.tree_build_begin(E.gaussian(3000, 10), 0.2, 0.1)
    try:
        assert _insert(ctx, room, cid, R, t, a, r) == CAPACITY and (a.value, r.value) == (-7, -7) and ctx.map_size(room) == 0
    finally:
        tid, _ = ctx.tree_build_end()
        ctx.tree_release(tid)
    assert _insert(ctx, room, cid, R, t, a, r) == 0 and (a.value, r.value) == (rows, rows)
    assert ctx.map_download_f32(room).tobytes() == before
    ctx.cloud_release(cid)


def test_full_size_count(ctx, maps):
    """three folds of 120 000 points: the counts only, against the host twin"""
    rng = np.random.default_rng(120)
    mid = maps(voxel=0.2, initial_rows=1 << 17)
    twin = capi.host_map_create(0.2, 1 << 17, 1 << 24)
    try:
        total = 0
        for f in range(3):
            d = rng.normal(size=(120000, 3))
            pts = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(2.0, 60.0, size=(120000, 1))
            R, t = E.random_pose(6 + f)
            got = fold(ctx, mid, pts, R, t)
            assert got == capi.host_map_insert(twin, pts, R, t)
            total += got[0]
        assert 120000 < total == ctx.map_size(mid) < 360000
    finally:
        capi.host_map_destroy(twin)


FOLD_SIZES = [1, 63, 64, 65, 257, 1025, 4097]
FOLD_VOXELS = [1e-3, 0.1, 0.5, 50.0, 1e6]
FOLD_POSES = {"identity": E.IDENTITY, "random": E.random_pose(11)}


@pytest.mark.parametrize("n", FOLD_SIZES)
def test_thinned_export_is_a_first_fold(ctx, n):
    """cloud_export_f32 at voxel > 0: the bytes of a fresh map's first fold of the same cloud, downloaded"""
    for name, pts in E.input_sets(n, 100 + n):
        cid = ctx.cloud_upload(pts)
        try:
            for pose in sorted(FOLD_POSES):
                R, t = FOLD_POSES[pose]
                for voxel in FOLD_VOXELS:
                    mid = ctx.map_create(voxel, n, 1 << 24)
                    try:
                        ctx.map_insert_cloud(mid, cid, R, t)
                        want = ctx.map_download_f32(mid)
                    finally:
                        ctx.map_release(mid)
                    assert ctx.cloud_export_f32(cid, R, t, voxel).tobytes() == want.tobytes(), (name, pose, voxel)
        finally:
            ctx.cloud_release(cid)


def test_exports_between_folds_do_not_show(ctx, maps):
    """fold A, export B (voxel 0.5 and 0), fold B, export A, fold C on a map that grows: the map equals a restatement that never saw
    an export after every fold, every export its own — the shared scratch carries nothing from one call into the next, and an export
    settles nothing in a live table"""
    mid = maps(initial_rows=1)
    ref = V.RefMap(V.VOXEL)
    clouds = [(E.gaussian(4097, 500 + k, scale=5.0 + k), E.random_pose(70 + k)) for k in range(3)]
    cids = [ctx.cloud_upload(pts) for pts, _ in clouds]

    def fold_k(k):
        pts, (R, t) = clouds[k]
        added = ref.insert(pts, R, t)
        assert ctx.map_insert_cloud(mid, cids[k], R, t) == (added, ref.size)
        assert E.same_bits(ctx.map_download_f32(mid), ref.rows())

    def export_k(k, voxel):
        pts, (R, t) = clouds[k]
        assert E.same_bits(ctx.cloud_export_f32(cids[k], R, t, voxel), E.export_f32(pts, R, t, voxel))

    try:
        fold_k(0)
        export_k(1, 0.5)
        export_k(1, 0.0)
        fold_k(1)
        export_k(0, 0.5)
        fold_k(2)
        assert ref.size > 4097
    finally:
        for cid in cids:
            ctx.cloud_release(cid)
