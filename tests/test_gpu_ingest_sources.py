"""The device ingest of several sensors' records into one cloud — fe::sources_mark / records_range / sources_scatter through
madicp_cloud_ingest_sources — against the host twin madicp_host_ingest_sources (and the numpy restatement of
tests/ingest_sources_ref.py) over the case table, bit for bit (uint64 views, NaN positions separately); the merged cloud under
madicp_cloud_deskew_own_stamps; the refusals.  No tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

import deskew_stamped_ref as DR
import ingest_records_ref as R
import ingest_sources_ref as SR
from fixtures import B_MAX, B_MIN
from mad_icp_amd import capi, synth

pytestmark = pytest.mark.gpu

HZ = DR.HZ
INVALID, CAPACITY = -1, -4


def check(ctx, sources, t_range=None):
    """device == host twin == numpy reference: counts, points, stamps, range.  Returns (points, stamps or None, range, per source)."""
    ref_p, ref_s, ref_r, ref_per = SR.reference(sources, t_range)
    h_p, h_s, h_r, h_per = capi.host_ingest_sources(sources, t_range)
    cid, kept, rng, per = ctx.cloud_ingest_sources(sources, t_range)
    try:
        out = ctx.cloud_download(cid)
        if ref_s is None:
            st = None
            tmp, v = np.empty(kept), np.zeros(6)
            dp = C.POINTER(C.c_double)
            assert capi.hip_lib().madicp_cloud_stamps(ctx._h, cid, tmp.ctypes.data_as(dp), kept) == INVALID
            assert capi.hip_lib().madicp_cloud_deskew_own_stamps(ctx._h, cid, v.ctypes.data_as(dp), HZ, None) == INVALID
        else:
            st = ctx.cloud_stamps(cid)
    finally:
        ctx.cloud_release(cid)
    assert kept == out.shape[0] == h_p.shape[0] == ref_p.shape[0] and per == h_per == ref_per
    assert R.same_bits(out, h_p) and R.same_bits(out, ref_p)
    assert R.same_bits(np.array(rng), np.array(h_r)) and R.same_bits(np.array(rng), np.array(ref_r)), (rng, h_r, ref_r)
    if st is None:
        assert h_s is None
    else:
        assert R.same_bits(st, h_s) and R.same_bits(st, ref_s)
    return out, st, rng, per


@pytest.mark.parametrize("name", sorted(set(SR.CASES) - {"G"}))
def test_case_table(ctx, name):
    sources, t_range = SR.CASES[name]()
    out, st, rng, per = check(ctx, sources, t_range)
    if name == "A":  # one plain source IS madicp_cloud_ingest_records on the same buffer, in every bit
        s = sources[0]
        cid, kept, r1 = ctx.cloud_ingest_records(s.records, s.min_range, s.max_range, 0, layout=s.layout)
        try:
            assert kept == out.shape[0] and R.same_bits(ctx.cloud_download(cid), out) and R.same_bits(ctx.cloud_stamps(cid), st)
            assert R.same_bits(np.array(r1), np.array(rng))
        finally:
            ctx.cloud_release(cid)
    if name == "D":
        assert st is None and rng == (np.inf, -np.inf)
    if name == "F":
        assert per[0] == 0 and per[1] > 0 and rng[0] == 0.0 and st.min() > 0.0
    if name == "H":
        assert np.isnan(st).all()
    if name == "I":
        assert rng == t_range and st.min() < 0.0 and st.max() > 1.0
    if name == "M":
        assert per[0] > 200000 and per[1] > 0


def test_every_source_drops_everything(ctx):
    """case G: MADICP_ERR_INVALID, and no cloud (no id) was made on the way"""
    sources, _ = SR.CASES["G"]()
    good, _ = SR.CASES["B"]()
    before, _, _, _ = ctx.cloud_ingest_sources(good)
    _alive, arr, count, _ = SR.native_args(sources, None)
    cid, kept = C.c_int(-7), C.c_int64(-7)
    per, rng = np.full(8, -7, np.int64), np.full(2, -7.0)
    rc = capi.hip_lib().madicp_cloud_ingest_sources(ctx._h, arr, count, None, C.byref(cid), C.byref(kept), per.ctypes.data_as(C.POINTER(C.c_int64)),
                                                    rng.ctypes.data_as(C.POINTER(C.c_double)))
    assert rc == INVALID and cid.value == -7 and kept.value == -7 and (per == -7).all() and (rng == -7.0).all()
    with pytest.raises(capi.MadIcpError, match="survives"):
        ctx.cloud_ingest_sources(sources)
    after, _, _, _ = ctx.cloud_ingest_sources(good)
    assert after == before + 1                                         # the refused calls took no id: the cloud count is unchanged
    assert capi.host_ingest_sources(sources)[3] == [0, 0]
    for c in (before, after):
        ctx.cloud_release(c)


def test_optional_outputs_may_be_null(ctx):
    sources, _ = SR.CASES["B"]()
    h_p, h_s, _, _ = capi.host_ingest_sources(sources)
    _alive, arr, count, _ = SR.native_args(sources, None)
    cid, kept = C.c_int(-7), C.c_int64(-7)
    assert capi.hip_lib().madicp_cloud_ingest_sources(ctx._h, arr, count, None, C.byref(cid), C.byref(kept), None, None) == 0
    try:
        assert kept.value == h_p.shape[0]
        assert R.same_bits(ctx.cloud_download(cid.value), h_p) and R.same_bits(ctx.cloud_stamps(cid.value), h_s)
    finally:
        ctx.cloud_release(cid.value)


def test_exact_reassembly(ctx):
    """case L: a scan split into an identity source and a rotated, time-shifted one merges back into the single-source ingest"""
    scan = SR.quantised(synth.render_scan(synth.Scene(0), synth.path_pose(2.0), 7, n_beams=16, n_azimuth=450))
    rng = np.random.default_rng(50)
    xyz = np.insert(scan, rng.integers(0, scan.shape[0], size=40), np.full((40, 3), 400.0, np.float32), axis=0)
    ticks = rng.integers(SR.TIME_SHIFT, 10**8, size=xyz.shape[0]).astype("<u4")
    whole, sources = SR.reassembly(xyz, ticks)
    out, st, r, _ = check(ctx, sources)
    cid, kept, r1 = ctx.cloud_ingest_records(whole, SR.LO, SR.HI, 0, layout=SR.L22)
    try:
        p1, s1 = ctx.cloud_download(cid), ctx.cloud_stamps(cid)
    finally:
        ctx.cloud_release(cid)
    assert kept == out.shape[0] == scan.shape[0]
    assert np.array_equal(out, p1) and np.array_equal(st, s1) and r == r1


@pytest.mark.parametrize("vname", sorted(DR.VELOCITIES))
def test_deskew_own_stamps_on_the_merged_cloud(ctx, vname):
    """case E's merged cloud under madicp_cloud_deskew_own_stamps against madicp_host_deskew_stamped on the twin's output"""
    sources, _ = SR.CASES["E"]()
    Tp, Tn = DR.poses_for(DR.VELOCITIES[vname], HZ)
    h_p, h_s, _, _ = capi.host_ingest_sources(sources)
    h_out, v6, h_chunks = capi.host_deskew_stamped(h_p, h_s, Tp, Tn, HZ)
    cid, kept, _, _ = ctx.cloud_ingest_sources(sources)
    try:
        chunks = ctx.cloud_deskew_own_stamps(cid, v6, HZ, want_chunks=True)
        out = ctx.cloud_download(cid)
        assert R.same_bits(ctx.cloud_stamps(cid), h_s)                 # the cloud keeps its stamps
    finally:
        ctx.cloud_release(cid)
    assert np.array_equal(chunks, h_chunks) and len(set(chunks.tolist())) > 100
    assert R.same_bits(out, h_out)


def test_merged_cloud_builds_and_repeats_across_scratch_growth(ctx):
    """small, then the 35 MB of case M (the scratch grows), then small again — the same bits — and the merged cloud builds"""
    small, _ = SR.CASES["K"]()
    a = check(ctx, small)
    big, _ = SR.CASES["M"]()
    check(ctx, big)
    b = check(ctx, small)
    assert R.same_bits(a[0], b[0]) and R.same_bits(a[1], b[1])
    cid, kept, _, _ = ctx.cloud_ingest_sources(small)
    up = ctx.cloud_upload(a[0])
    t_dev, nl_dev = ctx.tree_build(cid, B_MAX, B_MIN)
    t_ref, nl_ref = ctx.tree_build(up, B_MAX, B_MIN)
    assert nl_dev == nl_ref
    assert ctx.tree_download(t_dev, 2 * nl_dev - 1).tobytes() == ctx.tree_download(t_ref, 2 * nl_ref - 1).tobytes()
    for t in (t_dev, t_ref):
        ctx.tree_release(t)
    for c in (cid, up):
        ctx.cloud_release(c)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals(ctx):
    L = capi.hip_lib()
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int64)
    cid, kept = C.c_int(-7), C.c_int64(-7)
    per, rng = np.full(16, -7, np.int64), np.full(2, -7.0)

    def call(sources, t_range=None, h=ctx._h, null=()):
        _alive, arr, count, tr = SR.native_args(sources, t_range)
        return L.madicp_cloud_ingest_sources(h, None if "sources" in null else arr, count, None if tr is None else tr.ctypes.data_as(dp),
                                             None if "id" in null else C.byref(cid), None if "n" in null else C.byref(kept),
                                             per.ctypes.data_as(ip), rng.ctypes.data_as(dp))

    good, _ = SR.CASES["B"]()
    first, _, _, _ = ctx.cloud_ingest_sources(good)
    assert call(good, h=None) == INVALID
    for null in ("sources", "id", "n"):
        assert call(good, null=(null,)) == INVALID, null
    _alive, arr, count, _ = SR.native_args(good, None)
    arr[1].data = None
    assert L.madicp_cloud_ingest_sources(ctx._h, arr, count, None, C.byref(cid), C.byref(kept), None, None) == INVALID
    for why, sources, t_range in SR.bad_source_sets():
        assert call(sources, t_range) == INVALID, why
    assert cid.value == -7 and kept.value == -7 and (per == -7).all() and (rng == -7.0).all()
    with pytest.raises(capi.MadIcpError, match="t_scale"):
        ctx.cloud_ingest_sources([SR.source(SR.L22, 300, 60, time_scale=0.0)])
    with pytest.raises(capi.MadIcpError, match="in every source or in none"):
        ctx.cloud_ingest_sources([good[0], SR.source((13, 1, 5, 9, 0, 0), 37, 62)])
    # a look-ahead build in flight owns the builder's scratch
    r = np.random.default_rng(32)
    d = r.normal(size=(2000, 3))
    ctx.tree_build_begin(np.ascontiguousarray(d / np.linalg.norm(d, axis=1, keepdims=True) * r.uniform(0.5, 40.0, (2000, 1))), B_MAX, B_MIN)
    try:
        assert call(good) == CAPACITY
        with pytest.raises(capi.MadIcpError, match="look-ahead tree build is in flight"):
            ctx.cloud_ingest_sources(good)
    finally:
        ctx.tree_build_cancel()
    assert cid.value == -7 and kept.value == -7
    second, _, _, _ = ctx.cloud_ingest_sources(good)
    assert second == first + 1                                         # none of the refused calls made a cloud
    for c in (first, second):
        ctx.cloud_release(c)
    check(ctx, good)                                                   # ... and the context still ingests correctly
