"""The per-point attribute on the device (include/madicp_hip.h: madicp_cloud_ingest_sources_attr, madicp_cloud_set_attr / _attr,
madicp_cloud_deskew's gather, madicp_cloud_export_f32_attr, madicp_map_create_attr / _download_attr — kernels fe::sources_scatter,
fe::attr_gather, fe::voxel_rows) against the numpy restatement of tests/attribute_ref.py and the host twins.  The attribute is
integer data that is only copied: every comparison is exact equality."""
import copy
import ctypes as C

import numpy as np
import pytest

import attribute_ref as A
import cloud_export_ref as E
import ingest_sources_ref as S
import voxel_map_ref as V
from mad_icp_amd import capi
from mad_icp_amd.records import RecordLayout

pytestmark = pytest.mark.gpu

INVALID, CAPACITY = -1, -4
_fp = C.POINTER(C.c_float)


def _without(src):
    s = copy.copy(src)
    s.attribute = None
    return s


# ---- ingest ----------------------------------------------------------------------------------------------------------------------------
def counts_of(step):
    """1, one tile exactly, one tile - 1 and + 1, and enough for the survivors' scan to cross a 1 024 tile"""
    t = S.per_tile(step)
    return [1, t, t - 1, t + 1, 2500]


def make_sources(n_sources, which, keep_kind, seed):
    """sources over ingest_sources_ref.E_LAYOUTS whose record counts walk counts_of(): over the five values of `which` every source
    takes every count, so the first and the last record of every source sits at a source boundary at every tile fill"""
    lays = S.E_LAYOUTS if n_sources == 8 else [S.E_LAYOUTS[1], S.E_LAYOUTS[5]]
    out = []
    for k, lay in enumerate(lays):
        n = counts_of(lay.point_step)[(which + k) % 5]
        rng = np.random.default_rng([seed, k, n])
        if keep_kind == "all":
            keep = np.ones(n, bool)
        elif keep_kind == "half":
            keep = rng.integers(2, size=n) != 0
        else:  # exactly one record of the whole frame: the last record of the last source
            keep = np.zeros(n, bool)
            keep[-1] = k == len(lays) - 1
        out.append(S.source(lay, n, seed + k, keep=keep, time_offset=0.001 * k, sensor_to_base=S.rigid(seed + k) if k % 2 else None))
    return out


@pytest.mark.parametrize("code", A.CODES)
@pytest.mark.parametrize("keep_kind", ["all", "half", "one"])
@pytest.mark.parametrize("n_sources", [2, 8])
def test_ingest(ctx, n_sources, keep_kind, code):
    for which in range(5):
        sources = A.with_attribute(make_sources(n_sources, which, keep_kind, 100 + 10 * which), code)
        want = A.ingest(sources)
        twin = capi.host_ingest_sources_attr(sources)
        if keep_kind == "one":
            assert want[0].shape[0] == 1
        cid, kept, rng, per = ctx.cloud_ingest_sources_attr(sources)
        pid, pkept, prng, pper = ctx.cloud_ingest_sources([_without(s) for s in sources])
        try:
            assert (kept, per) == (want[0].shape[0], want[3]) == (pkept, pper) and rng == prng == twin[2]
            pts, st, w = ctx.cloud_download(cid), ctx.cloud_stamps(cid), ctx.cloud_attr(cid)
            assert w.dtype == np.uint32 and np.array_equal(w, want[4]) and np.array_equal(w, twin[4]), (which, code)
            assert S.R.same_bits(pts, want[0]) and pts.tobytes() == twin[0].tobytes()
            # points and stamps are those of the call without the attribute
            assert pts.tobytes() == ctx.cloud_download(pid).tobytes() and st.tobytes() == ctx.cloud_stamps(pid).tobytes()
            with pytest.raises(capi.MadIcpError):
                ctx.cloud_attr(pid)
        finally:
            ctx.cloud_release(cid)
            ctx.cloud_release(pid)


def test_ingest_last_bytes_and_refusals(ctx):
    """the field in the last bytes of a 13-, 22-, 26- and 256-byte record (the last record's field ends where the buffer does), and
    what the entry refuses: no cloud is made"""
    for step in (13, 22, 26, 256):
        lay = RecordLayout(step, 0, 4, 8, 0, 0)
        for code in (2, 4, 7):
            sources = A.with_attribute([S.source(lay, S.per_tile(step) + 1, 300 + step)], code, last_bytes=True)
            cid, kept, _, _ = ctx.cloud_ingest_sources_attr(sources)
            try:
                assert np.array_equal(ctx.cloud_attr(cid), A.ingest(sources)[4])
            finally:
                ctx.cloud_release(cid)
    a, b = S.source(S.L22, 300, 60), S.source(S.L16, 200, 61)
    for fields in ([(3, 7), None], [None, (3, 7)], [(3, 7), (3, 6)], [(3, 8), (3, 8)], [(-1, 2), (0, 2)], [(19, 7), (3, 7)], [(3, 7), (13, 7)],
                   [(21, 3), (3, 3)]):
        sa, sb = copy.copy(a), copy.copy(b)
        sa.attribute, sb.attribute = fields
        with pytest.raises(capi.MadIcpError):
            ctx.cloud_ingest_sources_attr([sa, sb])


# ---- a column of the caller's, and the deskews -----------------------------------------------------------------------------------------
def distinct_azimuths(n, seed):
    rng = np.random.default_rng(seed)
    az = rng.permutation(np.linspace(-3.1, 3.1, n))
    r = rng.uniform(3.0, 30.0, n)
    return np.ascontiguousarray(np.stack([r * np.cos(az), r * np.sin(az), rng.uniform(-2.0, 2.0, n)], axis=1))


def test_set_attr_and_refusals(ctx):
    pts = E.gaussian(1000, 1)
    cid = ctx.cloud_upload(pts)
    try:
        with pytest.raises(capi.MadIcpError):
            ctx.cloud_attr(cid)
        with pytest.raises(capi.MadIcpError):
            ctx.cloud_set_attr(cid, A.hashed(999))
        with pytest.raises(capi.MadIcpError):
            ctx.cloud_export_f32_attr(cid, *E.IDENTITY, 0.0)
        with pytest.raises(capi.MadIcpError):
            ctx.cloud_set_attr(cid + 1000, A.hashed(1000))
        ctx.cloud_set_attr(cid, A.hashed(1000))
        assert np.array_equal(ctx.cloud_attr(cid), A.hashed(1000))
        ctx.cloud_set_attr(cid, A.hashed(1000, 5))  # (new words into the same column)
        assert np.array_equal(ctx.cloud_attr(cid), A.hashed(1000, 5))
        assert ctx.cloud_download(cid).tobytes() == pts.tobytes()
    finally:
        ctx.cloud_release(cid)


@pytest.mark.parametrize("n", [257, 2500])
def test_azimuth_deskew_takes_the_column_along(ctx, n):
    pts = distinct_azimuths(n, 7)
    perms = []
    for vel in (np.zeros(6), np.array([1.5, -0.4, 0.1, 0.02, -0.03, 0.3])):
        cid = ctx.cloud_upload(pts)
        try:
            ctx.cloud_set_attr(cid, np.arange(n, dtype=np.uint32))
            ctx.cloud_deskew(cid, vel, 10.0)
            out, w = ctx.cloud_download(cid), ctx.cloud_attr(cid)
            assert sorted(w.tolist()) == list(range(n))
            if not vel.any():  # the identity pose in every chunk: row j IS input point attr[j]
                assert out.tobytes() == np.ascontiguousarray(pts[w]).tobytes()
            perms.append(w)
        finally:
            ctx.cloud_release(cid)
    assert np.array_equal(perms[0], perms[1])  # the order is the azimuths', whatever the velocity
    az = np.arctan2(pts[perms[0], 1], pts[perms[0], 0])
    assert (np.diff(az) > 0).all()


def test_stamped_deskews_leave_the_column(ctx):
    n = 2500
    vel = np.array([1.5, -0.4, 0.1, 0.02, -0.03, 0.3])
    pts, stamps = distinct_azimuths(n, 8), np.random.default_rng(8).uniform(0.0, 1.0, n)
    cid = ctx.cloud_upload(pts)
    try:
        ctx.cloud_set_attr(cid, A.hashed(n))
        ctx.cloud_deskew_stamped(cid, stamps, vel, 10.0)
        assert np.array_equal(ctx.cloud_attr(cid), A.hashed(n)) and ctx.cloud_download(cid).tobytes() != pts.tobytes()
    finally:
        ctx.cloud_release(cid)
    sources = A.with_attribute(make_sources(2, 4, "half", 500), 6)
    cid, kept, _, _ = ctx.cloud_ingest_sources_attr(sources)
    try:
        before, st = ctx.cloud_attr(cid), ctx.cloud_stamps(cid)
        ctx.cloud_deskew_own_stamps(cid, vel, 10.0)
        assert np.array_equal(ctx.cloud_attr(cid), before) and ctx.cloud_stamps(cid).tobytes() == st.tobytes()
        ctx.cloud_deskew(cid, vel, 10.0)  # (the azimuth deskew drops the stamps and keeps the column)
        assert sorted(ctx.cloud_attr(cid).tolist()) == sorted(before.tolist())
        with pytest.raises(capi.MadIcpError):
            ctx.cloud_stamps(cid)
    finally:
        ctx.cloud_release(cid)


# ---- export ----------------------------------------------------------------------------------------------------------------------------
ONE_CELL_VOXEL = 1e6  # (every finite point of every set within one or a few cells; one_cell under the identity: exactly one)


@pytest.mark.parametrize("n", [1, 64, 65, 1025, 4097])
def test_export(ctx, n):
    attr = A.hashed(n, n)
    for name, pts in E.input_sets(n, 200 + n):
        R, t = E.IDENTITY if name in ("one_cell", "own_cells", "two_cells") else E.random_pose(n)
        cid = ctx.cloud_upload(pts)
        try:
            ctx.cloud_set_attr(cid, attr)
            for voxel in (0.0, 0.5, ONE_CELL_VOXEL):
                rows, w = ctx.cloud_export_f32_attr(cid, R, t, voxel)
                want_rows, want_w = A.export(pts, attr, R, t, voxel)
                assert E.same_bits(rows, want_rows) and np.array_equal(w, want_w), (name, voxel)
                assert rows.tobytes() == ctx.cloud_export_f32(cid, R, t, voxel).tobytes()
                twin = capi.host_cloud_export_f32_attr(pts, attr, R, t, voxel)
                assert rows.tobytes() == twin[0].tobytes() and np.array_equal(w, twin[1])
                again = ctx.cloud_export_f32_attr(cid, R, t, voxel)
                assert again[0].tobytes() == rows.tobytes() and again[1].tobytes() == w.tobytes()
                if name == "one_cell" and voxel > 0:
                    assert w.tolist() == [int(attr[0])]  # one row, and its word is point 0's
            assert np.array_equal(ctx.cloud_attr(cid), attr)  # (the cloud is only read)
        finally:
            ctx.cloud_release(cid)


def test_export_refusals_write_nothing(ctx):
    n = 100
    cid, bare = ctx.cloud_upload(E.own_cells(n)), ctx.cloud_upload(E.own_cells(n))
    try:
        ctx.cloud_set_attr(cid, A.hashed(n))
        Rm, tv = np.eye(3).reshape(9), np.zeros(3)
        out, ow, m = np.full((n, 3), 7.0, np.float32), np.full(n, 0xdeadbeef, np.uint32), C.c_int64(-5)
        call = lambda c, voxel, cap, o=ow: capi.hip_lib().madicp_cloud_export_f32_attr(  # noqa: E731
            ctx._h, c, Rm.ctypes.data_as(capi._dp), tv.ctypes.data_as(capi._dp), voxel, out.ctypes.data_as(_fp),
            o.ctypes.data_as(capi._u32p) if o is not None else None, cap, C.byref(m))
        assert call(bare, 0.5, n) == INVALID and call(cid + 1000, 0.5, n) == INVALID and call(cid, -1.0, n) == INVALID
        assert call(cid, 0.5, n, None) == INVALID and m.value == -5
        assert call(cid, 0.0, n - 1) == CAPACITY and m.value == n
        assert call(cid, 0.5, n - 1) == CAPACITY and m.value == n
        assert (out == 7.0).all() and (ow == 0xdeadbeef).all()
        assert call(cid, 0.5, n) == 0 and m.value == n and np.array_equal(ow, A.hashed(n))
    finally:
        ctx.cloud_release(cid)
        ctx.cloud_release(bare)


# ---- the map ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def maps(ctx):
    made = []

    def make(with_attr=True, voxel=V.VOXEL, initial_rows=1, max_rows=1 << 24):
        made.append((ctx.map_create_attr if with_attr else ctx.map_create)(voxel, initial_rows, max_rows))
        return made[-1]

    yield make
    for mid in made:
        ctx.map_release(mid)


def fold(ctx, mid, pts, attr, R, t):
    cid = ctx.cloud_upload(pts)
    try:
        if attr is not None:
            ctx.cloud_set_attr(cid, attr)
        return ctx.map_insert_cloud(mid, cid, R, t)
    finally:
        ctx.cloud_release(cid)


@pytest.mark.parametrize("kind", ["identity", "random"])
@pytest.mark.parametrize("n", [1, 65, 1025, 4097])
def test_map_sequences(ctx, maps, n, kind):
    """initial_rows = 1: the block grows (rows, keys AND the column move, the table is rehashed) at nearly every fold"""
    mid, plain, ref = maps(), maps(with_attr=False), A.AttrMap(V.VOXEL)
    twin = capi.host_map_create_attr(V.VOXEL, 1, 1 << 24)
    try:
        prev = 0
        for f, (pts, R, t, added, want) in enumerate(V.reference(n, kind)):
            attr = None if f == 1 else A.hashed(n, 1000 * f)  # (frame 1: a cloud without a column contributes zeros)
            assert ref.insert(pts, attr, R, t) == added
            assert fold(ctx, mid, pts, attr, R, t) == (added, want.shape[0]) == fold(ctx, plain, pts, None, R, t)
            assert capi.host_map_insert_attr(twin, pts, attr, R, t) == (added, want.shape[0])
            for first in (0, prev):
                rows, w = ctx.map_download_f32(mid, first), ctx.map_download_attr(mid, first)
                assert E.same_bits(rows, want[first:]) and rows.tobytes() == ctx.map_download_f32(plain, first).tobytes()
                assert w.dtype == np.uint32 and np.array_equal(w, ref.attr(first)), (f, first)
                assert np.array_equal(w, capi.host_map_download_attr(twin, first))
            if f == 1:
                assert not ctx.map_download_attr(mid, prev).any()
            prev = want.shape[0]
        assert prev > 0
        ctx.map_clear(mid)
        assert ctx.map_size(mid) == 0 and ctx.map_download_attr(mid).shape == (0,)
        pts, R, t, added, want = V.reference(n, kind)[0]
        assert fold(ctx, mid, pts, A.hashed(n, 77), R, t) == (added, added)
        again = A.AttrMap(V.VOXEL)
        again.insert(pts, A.hashed(n, 77), R, t)
        assert np.array_equal(ctx.map_download_attr(mid), again.attr())
    finally:
        capi.host_map_destroy(twin)


def test_map_first_word_stays(ctx, maps):
    R, t = E.IDENTITY
    mid = maps()
    pts = E.one_cell(4096, 1)
    assert fold(ctx, mid, pts, A.hashed(4096, 1), R, t) == (1, 1)
    assert fold(ctx, mid, pts, A.hashed(4096, 2), R, t) == (0, 1) and fold(ctx, mid, E.one_cell(4096, 2), A.hashed(4096, 3), R, t) == (0, 1)
    assert ctx.map_download_attr(mid).tolist() == [int(A.hashed(4096, 1)[0])]


def test_map_refusals_write_nothing(ctx, maps):
    R, t = E.IDENTITY
    mid, plain = maps(), maps(with_attr=False)
    n = 50
    for m_ in (mid, plain):
        assert fold(ctx, m_, E.own_cells(n), A.hashed(n), R, t) == (n, n)
    ow, m = np.full(n, 0xdeadbeef, np.uint32), C.c_int64(-5)
    call = lambda map_id, first, cap, o=ow: capi.hip_lib().madicp_map_download_attr(  # noqa: E731
        ctx._h, map_id, first, o.ctypes.data_as(capi._u32p) if o is not None else None, cap, C.byref(m))
    assert call(plain, 0, n) == INVALID and call(mid + 1000, 0, n) == INVALID and call(mid, -1, n) == INVALID
    assert call(mid, n + 1, n) == INVALID and call(mid, 0, n, None) == INVALID and m.value == -5
    assert call(mid, 0, n - 1) == CAPACITY and m.value == n
    assert call(mid, 10, n - 11) == CAPACITY and m.value == n - 10
    assert (ow == 0xdeadbeef).all()
    assert call(mid, n, 0) == 0 and m.value == 0 and (ow == 0xdeadbeef).all()
    assert call(mid, 0, n) == 0 and m.value == n and np.array_equal(ow, A.hashed(n))
    assert ctx.map_download_f32(plain).tobytes() == ctx.map_download_f32(mid).tobytes()
