"""The device ingest of raw point records with a time field — fe::sources_mark / records_range / sources_scatter through
madicp_cloud_ingest_records, the one plain source of the sources ingest — with madicp_cloud_stamps and
madicp_cloud_deskew_own_stamps on top of it.

Everything is held bit for bit (uint64 views, NaN positions separately) to two references at once: the numpy restatement of
tests/ingest_records_ref.py and the host twin madicp_host_ingest_records.  No tolerance anywhere.

Not tested: that releasing a cloud returns its stamps buffer to the context's pool BY A COUNTER — the pool's byte count is not
visible through the C ABI.  test_scratch_and_repeated_release runs the 50 ingest / release rounds and holds every result."""
import ctypes as C

import numpy as np
import pytest

import deskew_stamped_ref as DR
import ingest_records_ref as R
from fixtures import B_MAX, B_MIN
from mad_icp_amd import capi
from mad_icp_amd.records import T_NONE

pytestmark = pytest.mark.gpu

HZ = DR.HZ
INVALID, CAPACITY = -1, -4


def check(ctx, buf, lay, kitti, t_range=None, expect_kept=None):
    """device == numpy reference == host twin: count, points, stamps, range.  Returns (points, stamps or None)."""
    ref_p, ref_s, ref_r = R.reference(buf, lay, R.LO, R.HI, kitti, t_range)
    if expect_kept is not None:
        assert ref_p.shape[0] == expect_kept                           # (the reference itself does what the case is built for)
    h_p, h_s, h_r = capi.host_ingest_records(buf, R.LO, R.HI, kitti, layout=lay, t_range=t_range)
    cid, kept, rng = ctx.cloud_ingest_records(buf, R.LO, R.HI, kitti, layout=lay, t_range=t_range)
    try:
        out = ctx.cloud_download(cid)
        if lay.t_type == T_NONE:
            st = None
            L = capi.hip_lib()
            tmp, v = np.empty(kept), np.zeros(6)
            dp = C.POINTER(C.c_double)
            assert L.madicp_cloud_stamps(ctx._h, cid, tmp.ctypes.data_as(dp), kept) == INVALID
            assert L.madicp_cloud_deskew_own_stamps(ctx._h, cid, v.ctypes.data_as(dp), HZ, None) == INVALID
        else:
            st = ctx.cloud_stamps(cid)
    finally:
        ctx.cloud_release(cid)
    assert kept == ref_p.shape[0] == out.shape[0] == h_p.shape[0]
    assert R.same_bits(out, ref_p) and R.same_bits(out, h_p)
    assert R.same_bits(np.array(rng), np.array(ref_r)) and R.same_bits(np.array(rng), np.array(h_r)), (rng, ref_r, h_r)
    if st is None:
        assert ref_s is None and h_s is None
    else:
        assert R.same_bits(st, ref_s) and R.same_bits(st, h_s)
    return out, st


@pytest.mark.parametrize("kitti", [0, 1])
@pytest.mark.parametrize("name", sorted(R.LAYOUTS))
def test_layouts_counts_and_survivor_patterns(ctx, name, kitti):
    lay = R.LAYOUTS[name]
    for n in R.COUNTS:
        for pattern in R.PATTERNS:
            keep = R.survivors(pattern, n)
            xyz = R.patterned(keep, n)
            buf = R.pack(lay, xyz, R.generic_times(lay, n, n), seed=n)
            out, _ = check(ctx, buf, lay, kitti, expect_kept=int(keep.sum()))
            if not kitti:                                             # in input order
                assert np.array_equal(out, xyz[keep].astype(np.float64)), (n, pattern)


@pytest.mark.parametrize("kitti", [0, 1])
def test_past_one_strip_of_tile_sums(ctx, kitti):
    """263 169 records = 258 tiles of marks: tb_scan_top carries over its first strip of 256 tile sums (the case of
    tests/test_gpu_frontend_edges.py), on the 48-byte layout."""
    n = 263169
    lay = R.LAYOUTS["ouster48"]
    keep = np.random.default_rng(5).integers(7, size=n) == 0
    keep[260100:263100] = False
    assert keep[:260100].sum() > 30000 and keep[263100:].any() and 260100 < 262144 < 263100
    check(ctx, R.pack(lay, R.patterned(keep, 6), R.generic_times(lay, n, 6), seed=6), lay, kitti, expect_kept=int(keep.sum()))


def test_second_trip_of_the_tile_loop(ctx):
    """256 * 8 * 256 + 1 records of 22 bytes: 2 049 tiles of 256 records on at most 8 workgroups per CU of a 256-CU part — the
    last tile, ONE record long, is some workgroup's second trip; both time extremes sit in it and in the first record."""
    n = 256 * 8 * 256 + 1
    lay = R.LAYOUTS["xyzirt22"]
    keep = np.random.default_rng(9).integers(3, size=n) != 0
    keep[-1] = True
    times = R.generic_times(lay, n, 9)
    times[-1], times[0] = -1.0, 7.0
    _, st = check(ctx, R.pack(lay, R.patterned(keep, 9), times, seed=9), lay, 1, expect_kept=int(keep.sum()))
    assert st[-1] == 0.0


@pytest.mark.parametrize("family", sorted(R.TIME_FAMILIES))
def test_time_families(ctx, family):
    make, t_type = R.TIME_FAMILIES[family]
    for name in R.FAMILY_LAYOUT[t_type]:
        lay = R.LAYOUTS[name]
        for n in (1, 2, 257, 1025, 4096):                             # (257, 1025: a partial last tile at every tile size)
            for pattern in ("all", "alternating", "one_per_tile"):
                keep = R.survivors(pattern, n)
                if family == "u32_extremes_dropped" and n > 2:        # first lane of the first tile, last record of a partial tile
                    keep[0] = keep[-1] = False
                    keep[1] = True
                times = make(n, keep, np.random.default_rng([n, 3]))
                buf = R.pack(lay, R.patterned(keep, n), times, seed=n)
                cid, kept, rng = ctx.cloud_ingest_records(buf, R.LO, R.HI, 0, layout=lay)
                try:
                    chunks = ctx.cloud_deskew_own_stamps(cid, np.zeros(6), HZ, want_chunks=True)
                finally:
                    ctx.cloud_release(cid)
                _, st = check(ctx, buf, lay, 0, expect_kept=int(keep.sum()))
                assert np.array_equal(chunks, DR.chunk_of(st))
                if family == "equal" or n == 1:
                    assert np.isnan(st).all() and (chunks == 1023).all()
                if family == "u32_extremes_dropped" and n > 2:
                    assert rng == (0.0, 1e8) and st.min() > 0.0 and st.max() < 1.0
                if family == "f32_signed_zero_min" and n > 1:
                    assert rng[0] == 0.0 and not np.signbit(rng[0])
                if family == "u32_ns" and n > 1:
                    assert rng == (0.0, 1e8)
                    if keep[0]:                                       # (the maximum is in the FIRST record)
                        assert st[0] == 1.0


def test_explicit_range_narrower_than_the_data(ctx):
    lay = R.LAYOUTS["f64at18"]
    n = 1025
    keep = R.survivors("alternating", n)
    buf = R.pack(lay, R.patterned(keep, 5), R.generic_times(lay, n, 5), seed=5)
    tr = (1.7e9 + 0.03, 1.7e9 + 0.06)
    _, st = check(ctx, buf, lay, 1, t_range=tr)
    assert st.min() < 0.0 and st.max() > 1.0
    cid, _, rng = ctx.cloud_ingest_records(buf, R.LO, R.HI, 1, layout=lay, t_range=tr)
    try:
        assert rng == tr
        chunks = ctx.cloud_deskew_own_stamps(cid, DR.VELOCITIES["rodrigues"], HZ, want_chunks=True)
    finally:
        ctx.cloud_release(cid)
    assert np.array_equal(chunks, DR.chunk_of(st)) and (chunks[st < 0] == 0).all() and (chunks[st > 1] == 1023).all()


# ---- deskew by the cloud's own stamps ----------------------------------------------------------------------------------------------
def _stamped_scan(n, seed, lay_name="xyzirt22"):
    lay = R.LAYOUTS[lay_name]
    rng = np.random.default_rng(seed)
    keep = rng.integers(10, size=n) != 0
    xyz = R.patterned(keep, seed)
    times = R.generic_times(lay, n, seed)
    if lay.t_type == 7:
        times[rng.integers(n, size=5)] = np.nan
    return R.pack(lay, xyz, times, seed=seed), lay


@pytest.mark.parametrize("vname", sorted(DR.VELOCITIES))
def test_deskew_own_stamps_equals_upload_and_deskew_stamped(ctx, vname):
    buf, lay = _stamped_scan(5000, 3)
    Tp, Tn = DR.poses_for(DR.VELOCITIES[vname], HZ)
    h_p, h_s, _ = capi.host_ingest_records(buf, R.LO, R.HI, 1, layout=lay)
    h_out, v6, h_chunks = capi.host_deskew_stamped(h_p, h_s, Tp, Tn, HZ)
    cid, kept, _ = ctx.cloud_ingest_records(buf, R.LO, R.HI, 1, layout=lay)
    pts, st = ctx.cloud_download(cid), ctx.cloud_stamps(cid)
    own_chunks = ctx.cloud_deskew_own_stamps(cid, v6, HZ, want_chunks=True)
    own = ctx.cloud_download(cid)
    assert R.same_bits(ctx.cloud_stamps(cid), st)                      # the cloud keeps its stamps: input order is kept
    ctx.cloud_release(cid)
    up = ctx.cloud_upload(pts)
    up_chunks = ctx.cloud_deskew_stamped(up, st, v6, HZ, want_chunks=True)
    ref = ctx.cloud_download(up)
    ctx.cloud_release(up)
    assert np.array_equal(own_chunks, up_chunks) and np.array_equal(own_chunks, h_chunks)
    assert R.same_bits(own, ref) and R.same_bits(own, h_out)


def test_deskew_back_to_back_with_azimuth_and_built(ctx):
    """the two deskews share the pose table's place in the scratch; a cloud deskewed by its own stamps builds into the tree of
    the host twin's output, byte for byte"""
    buf, lay = _stamped_scan(6000, 21, "ouster48")
    Tp, Tn = DR.poses_for(DR.VELOCITIES["rodrigues"], HZ)
    h_p, h_s, _ = capi.host_ingest_records(buf, R.LO, R.HI, 0, layout=lay)
    h_out, v6, _ = capi.host_deskew_stamped(h_p, h_s, Tp, Tn, HZ)
    ca, _, _ = ctx.cloud_ingest_records(buf, R.LO, R.HI, 0, layout=lay)
    cc, _, _ = ctx.cloud_ingest_records(buf, R.LO, R.HI, 0, layout=lay)
    cb = ctx.cloud_upload(h_p)
    ctx.cloud_deskew_own_stamps(ca, v6, HZ)
    ctx.cloud_deskew(cb, v6, HZ)
    ctx.cloud_deskew_own_stamps(cc, v6, HZ)
    az_first = ctx.cloud_download(cb)
    assert R.same_bits(ctx.cloud_download(ca), h_out) and R.same_bits(ctx.cloud_download(cc), h_out)
    ctx.cloud_release(cb)
    cb = ctx.cloud_upload(h_p)
    ctx.cloud_deskew(cb, v6, HZ)                                      # (the azimuth path after a stamped one: the same cloud)
    assert R.same_bits(ctx.cloud_download(cb), az_first)
    t_dev, nl_dev = ctx.tree_build(ca, B_MAX, B_MIN)
    ch = ctx.cloud_upload(h_out)
    t_ref, nl_ref = ctx.tree_build(ch, B_MAX, B_MIN)
    assert nl_dev == nl_ref
    assert ctx.tree_download(t_dev, 2 * nl_dev - 1).tobytes() == ctx.tree_download(t_ref, 2 * nl_ref - 1).tobytes()
    for t in (t_dev, t_ref):
        ctx.tree_release(t)
    # the azimuth deskew SORTS the points: a stamped cloud loses its stamps there
    L = capi.hip_lib()
    dp = C.POINTER(C.c_double)
    n = ctx.cloud_size(cc)
    tmp = np.empty(n)
    ctx.cloud_deskew(cc, v6, HZ)
    assert L.madicp_cloud_stamps(ctx._h, cc, tmp.ctypes.data_as(dp), n) == INVALID
    assert L.madicp_cloud_deskew_own_stamps(ctx._h, cc, v6.ctypes.data_as(dp), HZ, None) == INVALID
    assert ctx.cloud_size(cc) == n
    for c in (ca, cb, cc, ch):
        ctx.cloud_release(c)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals(ctx):
    L = capi.hip_lib()
    dp = C.POINTER(C.c_double)
    lay = R.LAYOUTS["xyzirt22"]
    n = 300
    keep = R.survivors("alternating", n)
    buf = R.pack(lay, R.patterned(keep, 31), R.generic_times(lay, n, 31), seed=31)
    data = buf.ctypes.data_as(C.c_void_p)
    cid, kept = C.c_int(-7), C.c_int64(-7)

    def call(layout=lay, count=n, h=ctx._h, d=data, t_range=None, lay_null=False, id_null=False, n_null=False):
        cl = capi.RecordLayoutC(*layout)
        tr = None if t_range is None else np.array(t_range, np.float64)
        return L.madicp_cloud_ingest_records(h, d, count, None if lay_null else C.byref(cl), R.LO, R.HI, 0,
                                             None if tr is None else tr.ctypes.data_as(dp), None if id_null else C.byref(cid),
                                             None if n_null else C.byref(kept), None)

    assert call(h=None) == INVALID and call(d=None) == INVALID and call(lay_null=True) == INVALID
    assert call(id_null=True) == INVALID and call(n_null=True) == INVALID
    assert call(count=0) == INVALID and call(count=-1) == INVALID and call(count=2**30 + 1) == INVALID
    assert call(count=2**30) == INVALID                                # this entry's own bound: the sources rule would allow it
    for bad in [(11, 0, 4, 7, 0, 0), (257, 0, 4, 8, 0, 0), (22, -1, 4, 8, 18, 7), (22, 0, 19, 8, 18, 7), (22, 0, 4, 22, 18, 7),
                (22, 0, 4, 8, 19, 7), (22, 0, 4, 8, 15, 8), (22, 0, 4, 8, -1, 6), (22, 0, 4, 8, 18, 5), (22, 0, 4, 8, 18, 9)]:
        assert call(layout=bad) == INVALID, bad
    for tr in [(2.0, 1.0), (1.0, 1.0), (np.nan, 1.0), (0.0, np.inf), (-np.inf, 0.0)]:   # inverted, equal, non-finite
        assert call(t_range=tr) == INVALID, tr
    far = R.pack(lay, np.full((n, 3), 500.0, np.float32), R.generic_times(lay, n, 1))
    assert call(d=far.ctypes.data_as(C.c_void_p)) == INVALID           # no point survives
    assert cid.value == -7 and kept.value == -7                        # no cloud was created by any of them
    with pytest.raises(capi.MadIcpError, match="record layout"):
        ctx.cloud_ingest_records(buf, R.LO, R.HI, 0, layout=(22, 0, 4, 8, 19, 7))
    with pytest.raises(capi.MadIcpError, match="t_range"):
        ctx.cloud_ingest_records(buf, R.LO, R.HI, 0, layout=lay, t_range=(1.0, 1.0))
    # a look-ahead build in flight owns the builder's scratch
    good, _, _ = ctx.cloud_ingest_records(buf, R.LO, R.HI, 0, layout=lay)
    v6 = np.ascontiguousarray(DR.VELOCITIES["rodrigues"])
    rng = np.random.default_rng(32)
    d = rng.normal(size=(2000, 3))
    ctx.tree_build_begin(np.ascontiguousarray(d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.5, 40.0, (2000, 1))), B_MAX, B_MIN)
    try:
        assert call() == CAPACITY
        assert L.madicp_cloud_deskew_own_stamps(ctx._h, good, v6.ctypes.data_as(dp), HZ, None) == CAPACITY
        with pytest.raises(capi.MadIcpError, match="look-ahead tree build is in flight"):
            ctx.cloud_ingest_records(buf, R.LO, R.HI, 0, layout=lay)
    finally:
        ctx.tree_build_cancel()
    assert cid.value == -7
    # refusals of the deskew by own stamps; the cloud is untouched by all of them
    before = ctx.cloud_download(good)
    V = v6.ctypes.data_as(dp)
    assert L.madicp_cloud_deskew_own_stamps(None, good, V, HZ, None) == INVALID
    assert L.madicp_cloud_deskew_own_stamps(ctx._h, good, None, HZ, None) == INVALID
    assert L.madicp_cloud_deskew_own_stamps(ctx._h, 987654, V, HZ, None) == INVALID
    assert L.madicp_cloud_deskew_own_stamps(ctx._h, good, V, 0.0, None) == INVALID
    assert L.madicp_cloud_deskew_own_stamps(ctx._h, good, V, -10.0, None) == INVALID
    plain = ctx.cloud_upload(before)
    assert L.madicp_cloud_deskew_own_stamps(ctx._h, plain, V, HZ, None) == INVALID     # a cloud without stamps
    tmp = np.empty(before.shape[0] + 1)
    assert L.madicp_cloud_stamps(ctx._h, plain, tmp.ctypes.data_as(dp), before.shape[0]) == INVALID
    assert L.madicp_cloud_stamps(ctx._h, good, tmp.ctypes.data_as(dp), before.shape[0] + 1) == INVALID   # n mismatch
    assert L.madicp_cloud_stamps(ctx._h, good, None, before.shape[0]) == INVALID
    assert R.same_bits(ctx.cloud_download(good), before)
    ctx.cloud_release(plain)
    ctx.cloud_release(good)
    check(ctx, buf, lay, 0, expect_kept=int(keep.sum()))                # ... and the context still ingests correctly


# ---- scratch and buffers ----------------------------------------------------------------------------------------------------------
def test_scratch_and_repeated_release(ctx):
    """small, large (the scratch grows: 256-byte records ask for ten times the points' room), small again on one context and on
    a fresh one; then 50 rounds of ingest / release at 4 096 records (the stamps buffer goes back to the pool with the points
    every time: see the module docstring for what is not asserted)"""
    cases = [("xyzirt22", 500), ("cap256", 60000), ("odd13", 37), ("xyzirt22", 500)]
    fresh = capi.Context(0)
    try:
        for name, n in cases:
            lay = R.LAYOUTS[name]
            keep = np.random.default_rng(n).integers(3, size=n) != 0
            buf = R.pack(lay, R.patterned(keep, n), R.generic_times(lay, n, n), seed=n)
            a = check(ctx, buf, lay, 1, expect_kept=int(keep.sum()))
            b = check(fresh, buf, lay, 1)
            assert R.same_bits(a[0], b[0])
    finally:
        fresh.close()
    lay = R.LAYOUTS["ouster48"]
    n = 4096
    keep = R.survivors("alternating", n)
    buf = R.pack(lay, R.patterned(keep, 2), R.generic_times(lay, n, 2), seed=2)
    ref_p, ref_s, _ = R.reference(buf, lay, R.LO, R.HI, 0)
    for _ in range(50):
        cid, kept, _ = ctx.cloud_ingest_records(buf, R.LO, R.HI, 0, layout=lay)
        assert kept == ref_p.shape[0]
        ctx.cloud_release(cid)
    cid, kept, _ = ctx.cloud_ingest_records(buf, R.LO, R.HI, 0, layout=lay)
    assert R.same_bits(ctx.cloud_download(cid), ref_p) and R.same_bits(ctx.cloud_stamps(cid), ref_s)
    ctx.cloud_release(cid)
